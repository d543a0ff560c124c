"""EXTENSION: the floor-contact term on sole vertices (stages.{chamfer,marker}.losses.floor_penetration / floor_contact,
uuo_fit_set_floor) on the MI355X -- the fused closures against float64 autograd, the term switched off, the compact packing,
the operator-composed route, the refusals, and what video_mocap_floor.yaml buys on a capture with a floor."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from floor_ref64 import _contacts, _planes, _vids  # noqa: E402
from gpu_support import (W_ACCEL_C, W_ACCEL_M, W_FLOOR_C as W_CHAMFER, W_FLOOR_M as W_MARKER, W_LOCK_C, W_LOCK_M,  # noqa: E402,F401
                         W_OFFS, _fit_points as _fit, _inputs, _makers_contacts as _makers, _marker_x, _rel_err, _three_corners,
                         dev, smpl, smpl64)
from stage_ref64 import _heights64, ref_chamfer64 as _ref_chamfer, ref_marker64 as _ref_marker  # noqa: E402
from uuo_mocap_amd.body_model import sole_vertices  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

# W_CHAMFER, W_MARKER (100, 10), the weights of the parity checks.  The plane is put through the middle of the sole heights (below),
# so about half the points penetrate by centimetres: d loss / d z = 2 w pen / (F K) is then of the size of the data term's
# 2 w_data d / F per frame at these weights, and the check that the term matters (> 1e-2 of the gradient) is met with a wide margin.


def _points(tables, K):
    """[[left ids], [right ids]] with K points in all: the default three per foot (None in the config) at K = 6"""
    if K == 6:
        return None
    sv = sole_vertices(tables, per_foot=K // 2)
    return [[int(v) for v in sv[0]], [int(v) for v in sv[1]]]


def _cfg(tables=None, K=6, w_chamfer=0.0, w_marker=0.0, h_chamfer=0.0, h_marker=0.0, sigma=0.0, temporal=False, offs=False,
         pen=True, con=True, keys=True):
    cfg = packaged_config("video_mocap")
    for stage, w, h, wa, wl in (("chamfer", w_chamfer, h_chamfer, W_ACCEL_C, W_LOCK_C), ("marker", w_marker, h_marker, W_ACCEL_M, W_LOCK_M)):
        st = cfg["stages"][stage]
        if keys:
            if pen:
                st["losses"]["floor_penetration"] = w
            if con:
                st["losses"]["floor_contact"] = w
            st["floor_height"] = h
            st["floor_points"] = None if tables is None else _points(tables, K)
        if temporal:
            st["losses"]["joint_accel"] = wa
            st["losses"]["foot_lock"] = wl
    if offs:
        cfg["stages"]["marker"]["losses"]["latent_offsets"] = W_OFFS
    for k in ("chamfer", "part", "marker"):
        cfg["stages"][k]["robust_sigma"] = sigma
    return cfg


def _median_plane(smpl64, tables, pose, betas, root, trans, q=50.0):
    """a plane through the default sole points' heights at these parameters, at their q-th percentile (the median: half the
    points penetrate and the other half hover): both pieces of the term are on"""
    return float(np.percentile(_heights64(smpl64, pose, betas, root, trans, _vids(tables, 6)), q))


# settings toggled off and on: (sigma, joint_accel + foot_lock, latent_offsets)
SETTINGS = [(0.0, False, False), (0.05, False, False), (0.0, True, False), (0.0, False, True), (0.05, True, True)]


def _parity(smpl, smpl64, tables, dev, F, M, K, seed, settings):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts = _contacts(F, seed)
    vids, k_left = _vids(tables, K), K // 2
    md = markers.to(dev)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    # the planes: the sole heights of the evaluated point in float64, per closure kind (the chamfer stage's root is another);
    # _plane asserts the distance from every kink before anything is compared
    h_c, h_m = _planes(smpl64, tables, F, M, K, seed)
    xc = ChamferProblem(smpl, *args, root.to(dev), _cfg(keys=False)).pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    for sigma, temporal, offs in settings:
        kw = dict(tables=tables, K=K, h_chamfer=h_c, h_marker=h_m, sigma=sigma, temporal=temporal)
        if not offs:  # (the chamfer stage has no latent offsets)
            cfg, cfg0 = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, **kw), _cfg(**kw)
            prob = ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts)
            prob0 = ChamferProblem(smpl, *args, root.to(dev), cfg0, foot_contacts=contacts)
            assert prob.floor_on and prob.floor_pen == W_CHAMFER and prob.floor_con == W_CHAMFER and not prob0.floor_on
            assert prob.floor_kl == k_left and prob.floor_kr == K - k_left
            loss, grad, nn = prob.evaluate(xc)
            _, grad0, nn0 = prob0.evaluate(xc)
            assert torch.equal(nn, nn0), "the term must not change the assignment"
            lo, g_ref = _ref_chamfer(smpl64, cfg, markers, o_pose, o_betas, root, xc, nn, contacts, vids, k_left)
            g = grad.cpu().numpy()
            tag = ("chamfer", F, M, K, sigma, temporal)
            print("OBS floor parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                  % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), _rel_err(g, grad0.cpu().numpy())))
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, g_ref) < 2e-4, tag
            assert _rel_err(g, grad0.cpu().numpy()) > 1e-2, tag
        cfg, cfg0 = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, offs=offs, **kw), _cfg(offs=offs, **kw)
        for assign, bary in ((mvids, None), (i3, b3)):
            mk = {"bary": None if bary is None else bary.to(dev), "foot_contacts": contacts}
            pm = MarkerProblem(smpl, *args, assign.to(dev), cfg, **mk)
            pm0 = MarkerProblem(smpl, *args, assign.to(dev), cfg0, **mk)
            assert pm.floor_on and pm.floor_pen == W_MARKER and not pm0.floor_on and pm.has_offsets == offs
            xm = _marker_x(pm, pp, bp, rp, tp, dev, F, num_markers=M)
            lm, gm, _ = pm.evaluate(xm, want_nn=False)
            _, gm0, _ = pm0.evaluate(xm, want_nn=False)
            lo, g_ref = _ref_marker(smpl64, tables, cfg, markers, o_pose, o_betas, xm, assign, bary, contacts, vids, k_left, M)
            g = gm.cpu().numpy()
            tag = ("three-corner" if bary is not None else "one-hot", F, M, K, sigma, temporal, offs)
            print("OBS floor parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                  % (tag, abs(lm - lo) / abs(lo), _rel_err(g, g_ref), _rel_err(g, gm0.cpu().numpy())))
            np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, g_ref) < 2e-4, tag
            assert _rel_err(g, gm0.cpu().numpy()) > 1e-2, tag


def _seed(F, M, K):
    """the seed of a parity case: one for which _plane's float64 preconditions hold (checked on the host)"""
    return SEEDS.get((F, M, K), 500 + 37 * F + M + K)


SEEDS = {(1, 50, 6): 1593, (3, 50, 16): 1677, (7, 10, 6): 1775, (7, 50, 6): 1815, (300, 50, 6): 49656}


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("M,K", [(10, 6), (11, 6), (50, 6), (50, 16), (5, 2)])
@pytest.mark.parametrize("F", [1, 3, 7])
def test_floor_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, M, K):
    """Loss rtol 2e-5, gradient relative error < 2e-4 against float64 autograd, and the term changes the gradient by more than
    1e-2 relative -- chamfer, one-hot and three-corner marker closures; (M, K) = (10, 6) fills one round of 16 item slots
    exactly, (11, 6) spills into a second, (50, 6) takes the last round's idle slots, (50, 16) a fifth round, (5, 2) is the
    smallest set; sigma, joint_accel + foot_lock and latent_offsets off and on."""
    _parity(smpl, smpl64, tables, dev, F, M, K, _seed(F, M, K), SETTINGS)


def test_floor_closures_match_float64_autograd_300_frames(smpl, smpl64, tables, dev):
    """The same at F = 300, M = 50, K = 6, per closure; plain and with every setting on."""
    _parity(smpl, smpl64, tables, dev, 300, 50, 6, _seed(300, 50, 6), [SETTINGS[0], SETTINGS[-1]])


# ------------------------------------------------------------------------------------------------ 2. off is off


def test_off_is_off_and_on_is_deterministic(smpl, smpl64, tables, dev):
    """Keys absent == both weights 0, bit for bit on loss and gradient, for the three closure kinds, on a fresh thread's
    workspace and on one that has just evaluated with the term on; two evaluations with the term on are bitwise equal;
    floor_contact with zero (or no) contacts equals floor_penetration alone, and alone it is off."""
    F = 41
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, F, 123)
    contacts = _contacts(F, 5)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    tp, zp, bp, pp, rp = pert
    h = _median_plane(smpl64, tables, pp, bp, rp, tp)
    on = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, h_chamfer=h, h_marker=h)
    pen_only = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, h_chamfer=h, h_marker=h, con=False)
    con_only = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, h_chamfer=h, h_marker=h, pen=False)
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
        assert pw.floor_pen > 0.0 and pw.floor_con > 0.0
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)       # the term on this thread's workspace first
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name  # no float atomics
        lf, gf = fresh["r"]
        assert lw > lf and not torch.equal(gw, gf), name
        off = {"absent": (absent, contacts), "weights 0": (_cfg(h_chamfer=h, h_marker=h), contacts),
               "contact piece without contacts": (con_only, None), "contact piece, zero contacts": (con_only, torch.zeros(F, 2))}
        for tag, (cfg, fc) in off.items():
            p = make(cfg, fc)
            assert not p.floor_on, (name, tag)
            pw.evaluate(x, want_nn=False)               # the workspace has just run with the term on
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)
        pp_ = make(pen_only, contacts)
        assert pp_.floor_pen > 0.0 and pp_.floor_con == 0.0
        lp, gp, _ = pp_.evaluate(x, want_nn=False)
        assert lf < lp < lw, name
        for tag, fc in (("zero contacts", torch.zeros(F, 2)), ("no contacts", None)):
            p = make(on, fc)                            # floor_contact with nothing to act on arms weight 0
            assert p.floor_pen > 0.0 and p.floor_con == 0.0, (name, tag)
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lp and torch.equal(g0, gp), (name, tag)


# ------------------------------------------------------------------------------------------------ 3. compact packing
def test_third_rows_get_no_gradient_from_the_term(smpl, smpl64, tables, dev):
    """The term reaches the raw rotations through the Gram-Schmidt backward only: with reg_pose_body 0 the third rows' gradient
    entries are exact zeros, and a solve on the compact packing leaves them bit for bit."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F = 37
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 111)
    contacts = _contacts(F, 8)
    md = markers.to(dev)
    h = _median_plane(smpl64, tables, pp, bp, rp, tp)
    cfg = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, h_chamfer=h, h_marker=h)
    cfg["stages"]["chamfer"]["losses"]["reg_pose_body"] = 0.0
    cfg["stages"]["marker"]["losses"]["reg_pose_body"] = 0.0
    pc = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg, foot_contacts=contacts)
    assert pc.floor_on
    x = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    _, g, _ = pc.evaluate(x)
    gp = g[4 * F + 10:].reshape(F, 23, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any()
    third = x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2].clone()
    pc.solve(x, max_iter=10, lr=0.1)
    assert torch.equal(x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2], third)

    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, cfg, foot_contacts=contacts)
    assert pm.floor_on
    xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    _, g, _ = pm.evaluate(xm)
    gp = g[:207 * F].reshape(F, 23, 3, 3)
    groot = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any() and not groot[:, 2].any()
    third = xm[:207 * F].reshape(F, 23, 3, 3)[:, :, 2].clone()
    pm.solve(xm, max_iter=10, lr=1.0)
    assert torch.equal(xm[:207 * F].reshape(F, 23, 3, 3)[:, :, 2], third)


# ------------------------------------------------------------------------------------------------ 4. fused vs composed
@pytest.mark.parametrize("F", [7, 300])
def test_fused_and_composed_floor_solves_agree(smpl, smpl64, tables, dev, F):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.floor_fused: False): the start agrees to 1e-5, the end to 5e-2 / 8e-2
    (test_fused_and_composed_foot_lock_solves_agree's tolerances), and both decrease.
    The plane is a floor under the feet -- the 10th percentile of the start's sole heights, so the lowest tenth of the points
    penetrates and the feet in contact hover -- which is the term's use.  (A plane through the MEDIAN of the heights asks the
    body to fold its legs by centimetres; the term then outweighs the rest of the gradient twelve to one, 25 iterations end in
    mid-descent and where they end depends on the path: measured at F = 7, chamfer 1.954 -> 0.312 fused, 0.295 composed, 6 %
    apart, from a start that agrees to 1e-6.)  The weights are the stages' own data weights (10 and 1): a centimetre of floor
    error then weighs like a centimetre of marker error, as in a fit.  (At the parity checks' 100 and 10, ten times that, the
    term dominates the loss -- 3.91 of it at the start against 0.2 of data -- and the F = 7 solves end 3 % / 22 % apart; F = 300
    agreed at 0.2 % / 1.8 % there too.)"""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    M = 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F)
    contacts = _contacts(F, 9)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    h = _median_plane(smpl64, tables, o_pose, o_betas, root, trans, q=10.0)
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    out = {}
    for fused in (True, False):
        cfg = _cfg(w_chamfer=10.0, w_marker=1.0, h_chamfer=h, h_marker=h)
        cfg["execution"] = {"floor_fused": fused}
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
    print("OBS floor fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (F, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=8e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)
    assert final(cc) < first(cc) and final(mc) < first(mc)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_library_and_routes_refuse_the_term_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103)
    contacts = _contacts(F, 3)
    md = markers.to(dev)
    on = _cfg(w_chamfer=W_CHAMFER, w_marker=W_MARKER, h_chamfer=0.5, h_marker=0.5)
    sole = torch.from_numpy(sole_vertices(tables).reshape(-1).copy()).to(torch.int32).to(dev)
    cdev = contacts.to(dev).contiguous()

    def arm(p, w_pen=1.0, w_con=1.0):  # what no config can produce: the library itself must refuse it
        p.floor_vids, p.floor_kl, p.floor_kr, p.floor_contacts = sole, 3, 3, cdev
        p.floor_pen, p.floor_con, p.floor_height = w_pen, w_con, 0.0

    # the part stage refuses at evaluation
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    arm(pp)
    with pytest.raises(RuntimeError, match="part stage"):
        pp.evaluate(x)
    arm(pp, 0.0, 0.0)
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
    arm(ps, 0.0, 0.0)
    assert ps.evaluate(xs)[0] == ls0
    # the setter: every bad argument; off with null pointers
    lib, fit = smpl.device_model.lib, pp.fit
    V = smpl.device_model.V
    vp, cp = sole.data_ptr(), cdev.data_ptr()
    ok = lambda *a: lib.uuo_fit_set_floor(fit, *a)
    assert ok(1.0, 1.0, 0.0, vp, 3, 3, cp) == 0
    for w in (-1.0, float("nan"), float("inf")):
        assert ok(w, 1.0, 0.0, vp, 3, 3, cp) != 0 and ok(1.0, w, 0.0, vp, 3, 3, cp) != 0       # weights
    for hh in (float("nan"), float("inf"), -float("inf")):
        assert ok(1.0, 1.0, hh, vp, 3, 3, cp) != 0                                              # height
    big = torch.arange(20, dtype=torch.int32, device=dev)
    assert ok(1.0, 1.0, 0.0, big.data_ptr(), 9, 8, cp) != 0 and ok(1.0, 1.0, 0.0, big.data_ptr(), 16, 1, cp) != 0   # K > 16
    assert ok(1.0, 1.0, 0.0, big.data_ptr(), 8, 8, cp) == 0 and ok(1.0, 1.0, 0.0, big.data_ptr(), 1, 1, cp) == 0   # K = 16, 2
    assert ok(1.0, 1.0, 0.0, vp, 0, 3, cp) != 0 and ok(1.0, 1.0, 0.0, vp, 3, 0, cp) != 0        # a foot without points
    assert ok(1.0, 1.0, 0.0, vp, -1, 4, cp) != 0
    for bad_id in (V, -1):
        bad = sole.clone()
        bad[4] = bad_id
        assert ok(1.0, 1.0, 0.0, bad.data_ptr(), 3, 3, cp) != 0                                 # a vertex id outside [0, V)
    assert ok(1.0, 1.0, 0.0, None, 3, 3, cp) != 0
    assert ok(0.0, 1.0, 0.0, vp, 3, 3, None) != 0                                               # w_con > 0 with null contacts
    assert ok(1.0, 0.0, 0.0, vp, 3, 3, None) == 0                                               # the penetration piece needs none
    assert ok(0.0, 0.0, 0.0, None, 0, 0, None) == 0                                             # off, null pointers
    assert pp.evaluate(x)[0] == loss0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), on, foot_contacts=contacts)
    assert p.floor_on
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step.*floor_penetration / floor_contact"):
        solve_batch([p], [xc], max_iter=3)


# ------------------------------------------------------------------------------------------------ 6. what it buys


def _quality(out, seq, oracle_smpl):
    """(mean penetration, mean float in contact -- both against the TRUE contacts, in mm -- and mean vertex error in m)"""
    from uuo_mocap_amd.metrics import compute_floor_error

    r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
    sole = torch.from_numpy(np.asarray(seq.gt["sole_vids"]).reshape(-1).copy()).long()
    e = compute_floor_error(r["vertices"][:, sole, 2], 3, torch.from_numpy(np.asarray(seq.gt["foot_contacts"])),
                            seq.gt["floor_height"])
    return e["penetration_mm"], e["float_mm"], float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())


def test_floor_config(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic capture with planted feet on a floor (seed 0), once with all markers and once with the columns owned
    by joints 7, 8, 10, 11 removed (M = 46), fitted with video_mocap.yaml and with video_mocap_floor.yaml, measured against the
    true contacts and the true body.  First: the capture shows the failure (the plain fit is >= 1 mm off in penetration or float
    at M = 46).  Required: penetration and float each at most half the plain fit's, mean vertex error at most the plain fit's
    + 0.5 mm, on both captures.  And a capture without contacts, lifted a metre so that every sole point stays far above z = 0:
    the host cannot arm weight 0 for floor_penetration (it does not know the heights), so the *_fl kernels run and add zeros --
    the fit must agree with video_mocap.yaml's within the fused / composed tolerance (final losses at 5e-2 / 8e-2 relative);
    whether it is bit for bit as well is printed."""
    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50, planted_feet=True, floor=True)
    assert float(seq.img_smpl.foot_contacts.sum()) > 0
    full = np.asarray(seq.markers.get_points()).copy()
    owner = np.argmax(np.asarray(tables.lbs_weights)[np.asarray(seq.gt["marker_vids"])], axis=1)
    keep = ~np.isin(owner, [7, 8, 10, 11])
    assert keep.sum() == 46
    res = {}
    for tag, pts in (("all", full), ("nofeet", full[:, keep])):
        for name in ("video_mocap", "video_mocap_floor"):
            res[(tag, name)] = _quality(_fit(seq, pts, name, smpl, dev), seq, oracle_smpl)
            for k, v in zip(("penetration_mm", "float_mm", "vertex_m"), res[(tag, name)]):
                record_property("%s_%s_%s" % (tag, name, k), v)
        (p0, f0, v0), (p1, f1, v1) = res[(tag, "video_mocap")], res[(tag, "video_mocap_floor")]
        print("OBS floor (%s markers): penetration plain %.3f floor %.3f mm; float plain %.3f floor %.3f mm; vertex error plain "
              "%.2f floor %.2f mm" % (tag, p0, p1, f0, f1, 1e3 * v0, 1e3 * v1))
    p0, f0, _ = res[("nofeet", "video_mocap")]
    assert p0 >= 1.0 or f0 >= 1.0, "the capture does not show the failure: %r" % (res,)
    for tag in ("all", "nofeet"):
        (p0, f0, v0), (p1, f1, v1) = res[(tag, "video_mocap")], res[(tag, "video_mocap_floor")]
        assert p1 <= 0.5 * p0, (tag, res)
        assert f1 <= 0.5 * f0, (tag, res)
        assert v1 <= v0 + 5e-4, (tag, res)

    # a capture without video contacts whose sole points stay above the floor: floor_contact is armed with weight 0 and
    # floor_penetration adds zeros on other kernel instantiations (*_fl)
    from uuo_mocap_amd import multimodal

    plain = make_sequence(tables, seed=3, num_frames=24, num_markers=16)
    assert not plain.img_smpl.foot_contacts.any()
    pts = np.asarray(plain.markers.get_points()).copy()
    pts[..., 2] = np.where(np.abs(pts).sum(-1) != 0.0, pts[..., 2] + 1.0, 0.0)
    plain.img_smpl.trans[:, 2] += 1.0
    outs, stats = [], []
    for n in ("video_mocap", "video_mocap_floor"):
        outs.append(_fit(plain, pts, n, smpl, dev, iters=30))
        run = multimodal.LAST_RUN_STATS  # per stage, one statistics record per solve of the run
        stats.append((min(st["final_loss"] for st in run["chamfer"]), run["marker_final"][-1]["final_loss"]))
    same = all(torch.equal(torch.as_tensor(outs[0][k]), torch.as_tensor(outs[1][k])) for k in ("pose_body", "betas", "root_orient", "trans"))
    print("OBS floor config on a lifted capture without contacts: bit for bit like video_mocap.yaml: %s; final losses chamfer "
          "(best hypothesis) %.6e / %.6e, last marker solve %.6e / %.6e" % (same, stats[0][0], stats[1][0], stats[0][1], stats[1][1]))
    assert stats[1][0] == pytest.approx(stats[0][0], rel=5e-2)
    assert stats[1][1] == pytest.approx(stats[0][1], rel=8e-2)
