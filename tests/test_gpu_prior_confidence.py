"""EXTENSION: per-(frame, joint) weights on the video pose prior (stages.{chamfer,marker}.prior_confidence,
uuo_fit_set_prior_weights, k_prior_conf) on the MI355X -- the fused closures against float64 autograd, the term alone with its
exact zeros, switched off, the compact packing, the operator-composed route, the refusals, and video_mocap_dropout.yaml on a
capture whose video loses the person for three seconds."""
import copy
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capsules_ref64 import _caps_grad, _lists as _cap_lists  # noqa: E402
from floor_ref64 import _contacts, _vids  # noqa: E402
from gpu_support import (R_CHAMFER, R_MARKER, W_CAPS_C, W_CAPS_M, W_LIM_C, W_LIM_M, _fit, _inputs, _marker_x,  # noqa: E402,F401
                         _rel_err, _three_corners, dev, smpl, smpl64)
from joint_limits_ref64 import SETTINGS, SHAPES, _check_seed, _lim_grad, _seed  # noqa: E402
from prior_confidence_ref64 import _cfg, _prior64, _weight_tables, _without  # noqa: E402
from stage_ref64 import (_chamfer_forward64, _float64, _marker_forward64, ref_chamfer64 as _ref_chamfer,  # noqa: E402
                         ref_marker64 as _ref_marker)
from uuo_mocap_amd.body_model import smpl_joint_limits  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

# R_CHAMFER, R_MARKER (600, 60), the weights of the parity checks.  The evaluated pose is the target + 0.05 randn per entry
# (_inputs), so the uniform prior's gradient is 2 R 0.05 / (207 F) per entry, and the tables below change a third to a half of it: |weighted - uniform| ~ R 4e-3 / sqrt(F)
# over the pose entries.  The rest of the closure's float64 gradient at these points (data term, shape prior, and with the
# settings on the limit term at its weight of 10, the floor and the capsules) has a norm of up to 10 on the chamfer and 3 on the
# marker closures, measured in float64 on the host over every case below; with video_mocap.yaml's 1.0 / 0.1 the weights would
# move the whole gradient by 1e-4 or less.  The precondition asks for 2e-2, so the parity checks raise reg_pose_body, as the
# issue provides for: 600 / 60 give 3.9e-2 or more on the chamfer and one-hot closures of every case (float64, host).


def _compare(tag, loss, grad, l_rest, g_rest, x, pose_slice, o_pose, w, reg):
    """asserts the float64 precondition, then the parity of one evaluation"""
    n = g_rest.shape[0]
    lw, gw = _prior64(x, pose_slice, o_pose, w, reg, n)
    lu, gu = _prior64(x, pose_slice, o_pose, None, reg, n)
    differ = _rel_err(g_rest + gw, g_rest + gu)
    assert differ > 2e-2, ("the weighted and the uniform prior's gradients differ by %.2e only" % differ, tag)
    lo, g_ref = l_rest + lw, g_rest + gw
    g = grad.cpu().numpy()
    print("OBS prior confidence parity %s: loss rel %.2e, gradient rel %.2e, weighted vs uniform %.2e"
          % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), differ))
    np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
    assert _rel_err(g, g_ref) < 2e-4, tag


def _parity(smpl, smpl64, tables, dev, F, M, seed):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts = _contacts(F, seed)
    svids = _vids(tables, 6)
    md = markers.to(dev)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    planes = _check_seed(smpl64, tables, F, M, seed)   # the float64 preconditions of the limit, capsule and floor terms
    cap_list = _cap_lists(tables)["builder"]
    lim_tab = smpl_joint_limits()
    wtabs = _weight_tables(F, seed)
    xc = ChamferProblem(smpl, *args, root.to(dev), _cfg()).pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    n0 = 219 * F + 10
    sl_c, sl_m = slice(4 * F + 10, 211 * F + 10), slice(0, 207 * F)
    for sigma, temporal, floor, caps, offs in SETTINGS:
        for limits in (False, True):
            kw = dict(limits=limits, sigma=sigma, temporal=temporal, floor=planes if floor else None, caps=cap_list if caps else None)
            cfg, cfgm = _cfg(**kw), _cfg(offs=offs, **kw)
            rest = None
            for name, w in wtabs.items():
                prob = ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts, prior_weights=w)
                assert prob.prior_conf_on and prob.joint_limits_on == limits and prob.capsules_on == caps
                loss, grad, nn = prob.evaluate(xc)
                if rest is None:   # the float64 closure without the prior: once per setting, the tables share it
                    l0, g0 = _ref_chamfer(smpl64, _without(cfg), markers, o_pose, o_betas, root, xc, nn, contacts, svids, 3)
                    with _float64():
                        leaves, out = _chamfer_forward64(smpl64, xc.detach().cpu().double(), root.double(), F)
                    if caps:
                        lc, gc = _caps_grad(leaves, out, cap_list, W_CAPS_C)
                        l0, g0 = l0 + lc, g0 + gc
                    if limits:
                        lt, gt = _lim_grad(leaves, 3, lim_tab, W_LIM_C)
                        l0, g0 = l0 + lt, g0 + gt
                    rest = (l0, g0, nn)
                assert torch.equal(nn, rest[2]), "the weights must not change the assignment"
                _compare(("chamfer", name, F, M, sigma, temporal, floor, caps, limits), loss, grad, rest[0], rest[1], xc, sl_c,
                         o_pose, w, R_CHAMFER)
            for assign, bary in ((mvids, None), (i3, b3)):
                mk = {"bary": None if bary is None else bary.to(dev), "foot_contacts": contacts}
                rest = None
                for name, w in wtabs.items():
                    pm = MarkerProblem(smpl, *args, assign.to(dev), cfgm, prior_weights=w, **mk)
                    assert pm.prior_conf_on and pm.joint_limits_on == limits and pm.has_offsets == offs
                    xm = _marker_x(pm, pp, bp, rp, tp, dev, F, num_markers=M)
                    lm, gm, _ = pm.evaluate(xm, want_nn=False)
                    if rest is None:
                        l0, g0 = _ref_marker(smpl64, tables, _without(cfgm), markers, o_pose, o_betas, xm, assign, bary, contacts,
                                             svids, 3, M)
                        with _float64():
                            leaves, out = _marker_forward64(smpl64, xm.detach().cpu().double()[:n0], F)
                        pad = 3 * M if offs else 0
                        if caps:
                            lc, gc = _caps_grad(leaves, out, cap_list, W_CAPS_M, pad=pad)
                            l0, g0 = l0 + lc, g0 + gc
                        if limits:
                            lt, gt = _lim_grad(leaves, 0, lim_tab, W_LIM_M, pad=pad)
                            l0, g0 = l0 + lt, g0 + gt
                        rest = (l0, g0)
                    tag = ("three-corner" if bary is not None else "one-hot", name, F, M, sigma, temporal, floor, caps, offs, limits)
                    _compare(tag, lm, gm, rest[0], rest[1], xm, sl_m, o_pose, w, R_MARKER)


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("F,M", SHAPES)
def test_weighted_prior_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, M):
    """Loss rtol 2e-5, gradient relative error < 2e-4 against float64 autograd (test_gpu_floor's restatement of the closures
    without the pose prior, plus the capsules', the limit term's and the weighted prior's own, whose gradients add) -- chamfer,
    one-hot and three-corner closures; a run of frames at 0, hash-uniform weights in [0, 2] with exact zeros, per-joint weights;
    sigma, joint_accel + foot_lock, the floor term, the capsules and latent_offsets off and on, each with the joint-angle limit
    term off and on (the two share one buffer).  Asserted in float64 before anything is compared: the weighted and the uniform
    prior change the closure's gradient by more than 2e-2 relative."""
    _parity(smpl, smpl64, tables, dev, F, M, _seed(F, M))


# ------------------------------------------------------------------------------------------------ 2. the term alone
@pytest.mark.parametrize("F,M", SHAPES)
def test_the_term_alone_and_its_exact_zeros(smpl, tables, dev, F, M):
    """Data weight and reg_betas 0: loss and gradient ARE the weighted prior (float64, the tolerances of the parity check).
    Every pose entry of a (frame, joint) with weight 0 has a gradient that is exactly 0.0, and so has every third row that sits
    on its target (half of the joints' third rows are put there), whatever its weight."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seed = _seed(F, M)
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    md = markers.to(dev)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    pose = pp.clone()
    pose[:, ::2, 2, :] = o_pose[:, ::2, 2, :]     # third rows of the even body rows on their targets
    on_target = torch.zeros(F, 23, 3, 3, dtype=torch.bool)
    on_target[:, ::2, 2, :] = True
    cfg = _cfg()
    cfg["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_betas=0.0)
    cfg["stages"]["marker"]["losses"].update(marker=0.0, reg_betas=0.0)
    sl_c, sl_m = slice(4 * F + 10, 211 * F + 10), slice(0, 207 * F)
    for name, w in _weight_tables(F, seed).items():
        zero = (w == 0.0)[:, :, None, None].expand(F, 23, 3, 3)
        assert zero.any()    # (the run of zero frames is every frame at F = 1: loss and gradient are then exactly 0)
        cases = [("chamfer", ChamferProblem(smpl, *args, root.to(dev), cfg, prior_weights=w), sl_c, R_CHAMFER),
                 ("one-hot", MarkerProblem(smpl, *args, mvids.to(dev), cfg, prior_weights=w), sl_m, R_MARKER),
                 ("three-corner", MarkerProblem(smpl, *args, i3.to(dev), cfg, bary=b3.to(dev), prior_weights=w), sl_m, R_MARKER)]
        for kind, p, sl, reg in cases:
            assert p.prior_conf_on
            x = p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pose.to(dev)) if kind == "chamfer" else \
                p.pack(pose.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
            loss, grad, _ = p.evaluate(x, want_nn=False)
            lw, gw = _prior64(x, sl, o_pose, w, reg, p.n)
            g = grad.cpu().numpy()
            tag = (kind, name, F, M)
            print("OBS prior confidence alone %s: loss rel %.2e, gradient rel %.2e" % (tag, abs(loss - lw) / max(lw, 1e-30), _rel_err(g, gw)))
            np.testing.assert_allclose(loss, lw, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, gw) < 2e-4, tag
            gp = grad[sl].reshape(F, 23, 3, 3).cpu()
            assert bool((gp[zero] == 0.0).all()) and not gp[zero].any(), tag          # exact zeros, not rounding noise
            assert bool((gp[on_target] == 0.0).all()), tag
            assert zero.all() or bool((gp[~zero & ~on_target] != 0.0).any()), tag
            rest = torch.ones(p.n, dtype=torch.bool)
            rest[sl] = False
            assert not grad.cpu()[rest].any(), tag                                    # nothing but the prior is on


# ------------------------------------------------------------------------------------------------ 3. off is off
def _makers(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    tp, zp, bp, pp, rp = pert
    a = (md, o_pose.to(dev), o_betas.to(dev))
    return {
        "chamfer": (lambda c, w=None: ChamferProblem(smpl, *a, root.to(dev), c, prior_weights=w),
                    lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))),
        "marker": (lambda c, w=None: MarkerProblem(smpl, *a, vids.to(dev), c, prior_weights=w),
                   lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
        "marker3": (lambda c, w=None: MarkerProblem(smpl, *a, i3.to(dev), c, bary=b3.to(dev), prior_weights=w),
                    lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
    }


def test_off_is_off_and_on_is_deterministic(smpl, tables, dev):
    """No block, prior_weights=None (with and without the block) and a table of ones through Python are bit for bit the results
    of a fresh thread's workspace that never had the setting, also right after an evaluation with weights on the same
    workspace (weights, then null).  Ones armed directly through the C entry run k_prior_conf and agree with the plain closure
    within the parity tolerances.  Two evaluations with weights are bitwise equal."""
    F = 41
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, F, 123)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    block = packaged_config("video_mocap_dropout")
    w = _weight_tables(F, 7)["hash"]
    for name, (make, pack) in _makers(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert).items():
        fresh = {}

        def on_fresh_thread():  # workspaces are per thread: this one has never seen the setting
            p = make(absent)
            fresh["r"] = p.evaluate(pack(p), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        lf, gf = fresh["r"]
        pw = make(block, w)
        assert pw.prior_conf_on
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name  # fixed-order sums, no float atomics
        assert lw != lf and not torch.equal(gw, gf), name
        for tag, cfg, tab in (("no block", absent, None), ("block, no table", block, None), ("ones", block, torch.ones(F, 23)),
                              ("ones, no block", absent, torch.ones(F, 23))):
            p = make(cfg, tab)
            assert not p.prior_conf_on, (name, tag)
            pw.evaluate(x, want_nn=False)               # the workspace has just run with weights: then null restores the plain result
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)
        # ones armed directly (what the Python layer never does): k_prior_conf forms the uniform prior
        p1 = make(absent)
        p1.prior_weights = torch.ones(F, 23, device=dev)
        assert p1.prior_conf_on
        l1, g1, _ = p1.evaluate(x, want_nn=False)
        print("OBS prior confidence ones through the C entry (%s): loss rel %.2e, gradient rel %.2e"
              % (name, abs(l1 - lf) / abs(lf), _rel_err(g1.cpu().numpy(), gf.cpu().numpy())))
        np.testing.assert_allclose(l1, lf, rtol=2e-5)
        assert _rel_err(g1.cpu().numpy(), gf.cpu().numpy()) < 2e-4
        # reg_pose_body 0 with weights: allowed, changes nothing
        none = copy.deepcopy(absent)
        for stage in ("chamfer", "marker"):
            none["stages"][stage]["losses"]["reg_pose_body"] = 0.0
        a, b = make(none, w), make(none)
        assert a.prior_conf_on
        la, ga, _ = a.evaluate(x, want_nn=False)
        lb, gb, _ = b.evaluate(x, want_nn=False)
        assert la == lb and torch.equal(ga, gb), name


# ------------------------------------------------------------------------------------------------ 4. compact packing
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_compact_packing_with_weights(smpl, tables, dev, stage):
    """test_gpu_parity's check of the compact packing with weights on, and the solver's coordinate count (the debug flavour's
    uuo_debug_last_solve_n).  (a) Rows that start on their targets: the solve agrees with the full packing (UUO_NO_COMPACT=1, debug
    flavour) as there -- same losses to 1e-6, same counts, same iterate --, and no third row moves: the decision is taken from the
    problem's own w_pose and rows, not from the zeroed launch coefficient.  (b) A third row off its target in a frame of weight
    0, where it has no gradient: the solve is bit for bit the UUO_NO_COMPACT one, the path the same start takes without
    weights."""
    from uuo_mocap_amd import _lib
    from uuo_mocap_amd._lib import UuoLbfgsOptions, UuoLbfgsStats
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, _ptr, current_stream

    dbg = _lib.load_debug()
    F, M = 37, 18
    seq = make_sequence(tables, seed=31, num_frames=F, num_markers=M)
    cfg = packaged_config("video_mocap")
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).to(dev)
    root = seq.img_smpl.root_orient.to(dev)
    trans0 = torch.median(markers, dim=1)[0]
    w = torch.ones(F, 23)
    w[10:20] = 0.0
    w[:, 5] = 0.25

    def problem(weights):
        if stage == "chamfer":
            p = ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg, prior_weights=weights)
            return p, (lambda pose: p.pack(trans0, torch.zeros(F, 1, 1, device=dev), o_betas, pose)), 0.1, slice(4 * F + 10, 211 * F + 10)
        p = MarkerProblem(smpl, markers, o_pose, o_betas, torch.from_numpy(seq.gt["marker_vids"]).to(dev), cfg, prior_weights=weights)
        return p, (lambda pose: p.pack(pose, o_betas, root, trans0)), 1.0, slice(0, 207 * F)

    def solve(prob, lr, x0, no_compact):
        x = x0.clone()
        losses = []
        cb = _lib.EVAL_CALLBACK(lambda user, i, loss, d_x_eval: losses.append(loss))
        opt = UuoLbfgsOptions(40, 100, lr, 1e-7, 1e-9, 0, 0)
        st = UuoLbfgsStats()
        os.environ["UUO_NO_COMPACT"] = "1" if no_compact else "0"
        try:
            prob._arm()
            rc = dbg.uuo_lbfgs_solve(prob.fit, current_stream(dev), ctypes.byref(prob.problem), _ptr(x), ctypes.byref(opt),
                                     ctypes.byref(st), ctypes.cast(cb, ctypes.c_void_p), None)
        finally:
            os.environ.pop("UUO_NO_COMPACT", None)
        assert rc == 0, dbg.uuo_last_error()
        torch.cuda.synchronize()
        counts.append(dbg.uuo_debug_last_solve_n(prob.fit))
        return x, losses, (st.n_iter, st.n_eval, st.stop_reason)

    counts = []
    prob, pack, lr, sl = problem(w)
    assert prob.prior_conf_on
    third = torch.zeros(F, 23, 9, dtype=torch.bool, device=dev)
    third[..., 6:] = True
    x0 = pack(o_pose)
    xc, lc, sc = solve(prob, lr, x0, False)
    xf, lf, sf = solve(prob, lr, x0, True)
    head = min(len(lc), len(lf), 40)
    np.testing.assert_allclose(lc[:head], lf[:head], rtol=1e-6)
    assert abs(sc[0] - sf[0]) <= 2 and abs(sc[1] - sf[1]) <= 3, (sc, sf)
    assert float((xc - xf).abs().max()) < 1e-3
    for x in (xc, xf):
        assert torch.equal(x[sl].reshape(F, 23, 9)[third], x0[sl].reshape(F, 23, 9)[third])
    assert not torch.equal(xc, x0)
    # n_act is as today: 142 F + 10 (chamfer) / 147 F + 10 (marker) coordinates on the compact packing, the parameter count on the
    # full one (the two packings give bitwise equal iterates, DESIGN 4c, so the count is read from the workspace)
    n_compact = (142 if stage == "chamfer" else 147) * F + 10
    assert counts == [n_compact, prob.n] and n_compact < prob.n, (counts, n_compact, prob.n)
    # (b) one third row off its target, in a frame of weight 0
    pose_off = o_pose.clone()
    pose_off[12, 3, 2, :] += 0.01
    x1 = pack(pose_off)
    xa, la, sa = solve(prob, lr, x1, False)
    xb, lb, sb = solve(prob, lr, x1, True)
    assert torch.equal(xa, xb) and la == lb and sa == sb          # the full packing, as without the weights
    assert counts[2:] == [prob.n, prob.n], counts
    assert torch.equal(xa[sl].reshape(F, 23, 3, 3)[12, 3, 2], x1[sl].reshape(F, 23, 3, 3)[12, 3, 2])   # (no gradient: it stays)
    plain, pack0, _, _ = problem(None)
    ya, ma, ta = solve(plain, lr, pack0(pose_off), False)
    yb, mb, tb = solve(plain, lr, pack0(pose_off), True)
    assert torch.equal(ya, yb) and ma == mb and ta == tb          # (the same decision without them)
    assert counts[4:] == [plain.n, plain.n], counts
    solve(plain, lr, pack0(o_pose), False)
    assert counts[6] == n_compact, counts                         # (and the plain problem's count on its targets: as with weights)


# ------------------------------------------------------------------------------------------------ 5. fused vs composed
@pytest.mark.parametrize("F", [7, 300])
def test_fused_and_composed_weighted_solves_agree(smpl, tables, dev, F):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.prior_conf_fused: False) with a run of frames at 0 and tapered ends: the start agrees to 1e-5, the end to 5e-2,
    and both decrease (the bands of test_fused_and_composed_limit_solves_agree).  Both marker solves start from ONE point, the
    fused chamfer solve's result, so that their starts are comparable too (1e-5) and their ends measure the marker closures,
    not how far two unconverged chamfer solves had drifted apart: continued each from its own chamfer result (starts 0.6 % apart
    at F = 7) the marker ends after 25 iterations, a hundredfold decrease, were 7.6 % apart with the chamfer ends 0.7 % apart."""
    from uuo_mocap_amd.engine import prior_weight_table
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    M = 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    seen = torch.ones(F, dtype=torch.bool)
    seen[F // 3:F // 3 + max(2, F // 3)] = False
    w = prior_weight_table(seen, {"gap_weight": 0.1, "ramp": 2, "joint_weights": None})
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    out = {}
    start_m = None
    for fused in (True, False):
        cfg = packaged_config("video_mocap_dropout")
        cfg["execution"] = {"prior_conf_fused": fused}
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 25
        pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
        optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                      root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                      marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg,
                      prior_weights=w)
        sc = dict(last_stats("chamfer"))
        if start_m is None:   # (the fused route runs first)
            start_m = [t.detach().clone() for t in (pose, betas, rt, tr)]
        pose, betas, rt, tr = (t.clone().requires_grad_(True) for t in start_m)
        optim_markers(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                      trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                      smpl_inference=smpl, config=cfg, prior_weights=w)
        out[fused] = (sc, dict(last_stats("marker")))
    (cf, mf), (cc, mc) = out[True], out[False]
    assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
    print("OBS prior confidence fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (F, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert first(mf) == pytest.approx(first(mc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=5e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)
    assert final(cc) < first(cc) and final(mc) < first(mc)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_library_and_routes_refuse_the_weights_where_they_are_not_built(smpl, tables, dev):
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch
    from uuo_mocap_amd.optimization import optim_chamfer

    F, M = 9, 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103)
    md = markers.to(dev)
    w = _weight_tables(F, 3)["hash"].to(dev)
    # the part stage refuses at evaluation (what no config can produce: the library itself must refuse it)
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    pp.prior_weights = w
    with pytest.raises(RuntimeError, match="part stage"):
        pp.evaluate(x)
    pp.prior_weights = None
    assert pp.evaluate(x)[0] == loss0
    # the soft chamfer closure refuses at evaluation
    soft = packaged_config("video_mocap")
    soft["stages"]["chamfer"]["losses"]["soft_chamfer"] = 10.0
    ps = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft)
    xs = ps.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    ls0 = ps.evaluate(xs)[0]
    ps.prior_weights = w
    with pytest.raises(RuntimeError, match="soft-assignment"):
        ps.evaluate(xs)
    ps.prior_weights = None
    assert ps.evaluate(xs)[0] == ls0
    with pytest.raises(NotImplementedError, match="soft"):
        ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft, prior_weights=w)
    # the setter: -22 for a null workspace, 0 for null weights
    lib = smpl.device_model.lib
    assert lib.uuo_fit_set_prior_weights(None, None) == -22
    assert lib.uuo_fit_set_prior_weights(pp.fit, None) == 0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), packaged_config("video_mocap"), prior_weights=w)
    assert p.prior_conf_on
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step.*prior_confidence"):
        solve_batch([p], [xc], max_iter=3)
    # frame sharding
    pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="prior_confidence.*frame-block sharding"):
            optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, img_mask=torch.ones(F, device=dev), marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev),
                          smpl_inference=smpl, config=packaged_config("video_mocap"), prior_weights=w)


# ------------------------------------------------------------------------------------------------ 7. the shipped config


def test_dropout_config(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic capture (seed 0) whose video loses the person for frames 100 .. 189 (video_dropout=True), fitted with
    video_mocap.yaml and with video_mocap_dropout.yaml: the mean vertex error inside and outside the window is reported
    (record_property); required: outside the window the error stays within 0.5 mm of the plain fit's.  The default capture,
    whose mask is all True, builds a table of ones: its fit is bit-identical to the plain config's.  Measured with the shipped
    0.0 / 0: inside the window 21.73 -> 19.58 mm, outside it 19.17 -> 19.16 mm."""
    from uuo_mocap_amd.metrics import compute_window_vertex_error

    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50, video_dropout=True)
    window = seq.gt["dropout_window"]
    res = {}
    for name in ("video_mocap", "video_mocap_dropout"):
        out = _fit(seq, name, smpl, dev)
        r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                        out["trans"].cpu().float())
        res[name] = compute_window_vertex_error(r["vertices"], torch.from_numpy(seq.gt["verts"]), window)
        for k in ("inside", "outside"):
            record_property("%s_%s_vertex_m" % (name, k), res[name][k])
    print("OBS prior confidence (dropout capture): vertex error inside the window plain %.2f weighted %.2f mm; outside plain %.2f "
          "weighted %.2f mm" % tuple(1e3 * v for v in (res["video_mocap"]["inside"], res["video_mocap_dropout"]["inside"],
                                                      res["video_mocap"]["outside"], res["video_mocap_dropout"]["outside"])))
    assert res["video_mocap_dropout"]["outside"] <= res["video_mocap"]["outside"] + 5e-4, res
    base = make_sequence(tables, seed=0, num_frames=300, num_markers=50)
    a, b = _fit(base, "video_mocap", smpl, dev), _fit(base, "video_mocap_dropout", smpl, dev)
    for k in ("pose_body", "betas", "root_orient", "trans"):
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
