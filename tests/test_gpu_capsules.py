"""EXTENSION: the bone-capsule self-penetration term (stages.{chamfer,marker}.losses.self_penetration, uuo_fit_set_capsules) on
the MI355X -- the fused closures against float64 autograd, the term alone, switched off, the compact packing, the
operator-composed route, the refusals, and what video_mocap_capsules.yaml buys on a capture whose HMR start has an arm in the
torso."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capsules_ref64 import _caps_grad, _cfg, _check_seed, _lists  # noqa: E402
from floor_ref64 import _contacts, _vids  # noqa: E402
from gpu_support import (W_CAPS_C as W_CHAMFER, W_CAPS_M as W_MARKER, _fit, _inputs, _makers, _marker_x, _rel_err,  # noqa: E402,F401
                         _three_corners, dev, smpl, smpl64)
from stage_ref64 import (_chamfer_forward64, _float64, _marker_forward64, ref_chamfer64 as _ref_chamfer,  # noqa: E402
                         ref_marker64 as _ref_marker)
from uuo_mocap_amd.body_model import body_capsules  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

# W_CHAMFER, W_MARKER (100, 10), the weights of the parity checks.  With doubled radii the overlaps are centimetres deep; one pair's
# d loss / d c = 2 w pen / F is then 2 * 100 * 0.03 / F = 6 / F, against the data term's 2 w_data d / (F M) ~ 2 * 10 * 0.03 / (50 F)
# per marker: the check that the term matters (> 2e-2 of the gradient, a hundred times the tolerance) is met with a wide margin even
# by a single pair.

# seeds of the parity cases, chosen on the host: the first of 600 + 37 F + M + 1000 n (n = 0, 1, ...) that meets _check_seed
# (n = 1 for M = 11: a pair within 1e-4 m of its hinge at F = 1, a foot's two lowest sole points within 1e-4 m at F = 3 and 7)
SEEDS = {(1, 11): 1648, (3, 11): 1722, (7, 11): 1870}


def _seed(F, M):
    return SEEDS.get((F, M), 600 + 37 * F + M)


# settings toggled off and on: (sigma, joint_accel + foot_lock, the floor term, latent_offsets)
SETTINGS = [(0.0, False, False, False), (0.05, True, False, False), (0.0, False, True, True), (0.05, True, True, True)]


def _parity(smpl, smpl64, tables, dev, F, M, seed, alone=False):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts = _contacts(F, seed)
    svids = _vids(tables, 6)
    md = markers.to(dev)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    planes = _check_seed(smpl64, tables, F, M, seed)   # asserts every precondition before anything is compared
    all_lists = _lists(tables)
    xc = ChamferProblem(smpl, *args, root.to(dev), _cfg(keys=False)).pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    n0 = 219 * F + 10
    for si, (sigma, temporal, floor, offs) in enumerate([SETTINGS[0]] if alone else SETTINGS):
        for name, lists in all_lists.items():
            if si > 0 and name != "builder":
                continue
            kw = dict(sigma=sigma, temporal=temporal, floor=planes if floor else None)
            cfg, cfg0 = _cfg(lists, W_CHAMFER, W_MARKER, **kw), _cfg(lists, **kw)
            cfgm, cfgm0 = _cfg(lists, W_CHAMFER, W_MARKER, offs=offs, **kw), _cfg(lists, offs=offs, **kw)
            if alone:  # no data term, no priors: loss and gradient ARE the term
                for c in (cfg, cfg0, cfgm, cfgm0):
                    c["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_pose_body=0.0, reg_betas=0.0)
                    c["stages"]["marker"]["losses"].update(marker=0.0, reg_pose_body=0.0, reg_betas=0.0)
            prob = ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts)
            prob0 = ChamferProblem(smpl, *args, root.to(dev), cfg0, foot_contacts=contacts)
            assert prob.capsules_on and prob.cap_w == W_CHAMFER and not prob0.capsules_on
            assert prob.cap_joints.shape[0] == len(lists[0]) and prob.cap_pairs.shape[0] == len(lists[2])
            loss, grad, nn = prob.evaluate(xc)
            _, grad0, nn0 = prob0.evaluate(xc)
            assert torch.equal(nn, nn0), "the term must not change the assignment"
            l0, g0 = _ref_chamfer(smpl64, cfg0, markers, o_pose, o_betas, root, xc, nn, contacts, svids, 3)
            with _float64():
                leaves, out = _chamfer_forward64(smpl64, xc.detach().cpu().double(), root.double(), F)
            lt, gt = _caps_grad(leaves, out, lists, W_CHAMFER)
            lo, g_ref = l0 + lt, g0 + gt
            g = grad.cpu().numpy()
            tag = ("chamfer", name, F, M, sigma, temporal, floor, alone)
            share = _rel_err(g, grad0.cpu().numpy())
            print("OBS capsules parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                  % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), share))
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, g_ref) < 2e-4, tag
            assert share > 2e-2, tag
            if alone:
                assert l0 == 0.0 and not g0.any()
            for assign, bary in ((mvids, None), (i3, b3)):
                mk = {"bary": None if bary is None else bary.to(dev), "foot_contacts": contacts}
                pm = MarkerProblem(smpl, *args, assign.to(dev), cfgm, **mk)
                pm0 = MarkerProblem(smpl, *args, assign.to(dev), cfgm0, **mk)
                assert pm.capsules_on and pm.cap_w == W_MARKER and not pm0.capsules_on and pm.has_offsets == offs
                xm = _marker_x(pm, pp, bp, rp, tp, dev, F, num_markers=M)
                lm, gm, _ = pm.evaluate(xm, want_nn=False)
                _, gm0, _ = pm0.evaluate(xm, want_nn=False)
                l0, g0 = _ref_marker(smpl64, tables, cfgm0, markers, o_pose, o_betas, xm, assign, bary, contacts, svids, 3, M)
                with _float64():
                    leaves, out = _marker_forward64(smpl64, xm.detach().cpu().double()[:n0], F)
                lt, gt = _caps_grad(leaves, out, lists, W_MARKER, pad=3 * M if offs else 0)
                lo, g_ref = l0 + lt, g0 + gt
                g = gm.cpu().numpy()
                tag = ("three-corner" if bary is not None else "one-hot", name, F, M, sigma, temporal, floor, offs, alone)
                share = _rel_err(g, gm0.cpu().numpy())
                print("OBS capsules parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                      % (tag, abs(lm - lo) / abs(lo), _rel_err(g, g_ref), share))
                np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=str(tag))
                assert _rel_err(g, g_ref) < 2e-4, tag
                assert share > 2e-2, tag


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("M", [10, 11, 50])
@pytest.mark.parametrize("F", [1, 3, 7])
def test_capsule_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, M):
    """Loss rtol 2e-5, gradient relative error < 2e-4 against float64 autograd (test_gpu_floor's restatement of the closures
    plus the term's own, whose gradients add), and the term changes the gradient by more than 2e-2 relative -- chamfer, one-hot
    and three-corner closures; the four lists (C, P) = (2, 1), the builder's (24, 232), its first 65 pairs, (32, 256) with
    spheres, radii doubled; sigma, joint_accel + foot_lock, the floor term and latent_offsets off and on (the builder's list).
    The float64 preconditions of the issue are asserted first (_check_seed)."""
    _parity(smpl, smpl64, tables, dev, F, M, _seed(F, M))


@pytest.mark.parametrize("M", [10, 11, 50])
@pytest.mark.parametrize("F", [1, 3, 7])
def test_the_term_alone_matches_float64(smpl, smpl64, tables, dev, F, M):
    """The same shapes and the four lists with w_data = 0 and both priors 0: loss and gradient ARE the term (chamfer, one-hot
    and three-corner); the other settings stay off, since with them the closure is no longer the term alone."""
    _parity(smpl, smpl64, tables, dev, F, M, _seed(F, M), alone=True)


# ------------------------------------------------------------------------------------------------ 2. off is off


def test_off_is_off_and_on_is_deterministic(smpl, tables, dev):
    """Key absent == weight 0, bit for bit on loss and gradient, for the three closure kinds, on a fresh thread's workspace and
    on one that has just evaluated with the term on (w = 0 after w > 0); two evaluations with the term on are bitwise equal; a
    second list on the same workspace replaces the first (the library compares and uploads)."""
    F = 41
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, F, 123)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    lists = _lists(tables)
    on, on2 = _cfg(lists["builder"], W_CHAMFER, W_MARKER), _cfg(lists["cut65"], W_CHAMFER, W_MARKER)
    for name, (make, pack) in _makers(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert).items():
        fresh = {}

        def on_fresh_thread():  # workspaces are per thread: this one has never seen the term
            p = make(absent)
            fresh["r"] = p.evaluate(pack(p), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        pw = make(on)
        assert pw.capsules_on
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name  # no float atomics
        lf, gf = fresh["r"]
        assert lw > lf and not torch.equal(gw, gf), name
        p2 = make(on2)
        l2, g2, _ = p2.evaluate(x, want_nn=False)
        assert lf < l2 < lw, name                       # 65 of the 232 pairs
        lw3, gw3, _ = pw.evaluate(x, want_nn=False)      # and back
        assert lw3 == lw and torch.equal(gw3, gw), name
        for tag, cfg in (("absent", absent), ("weight 0", _cfg(lists["builder"]))):
            p = make(cfg)
            assert not p.capsules_on, (name, tag)
            pw.evaluate(x, want_nn=False)               # the workspace has just run with the term on
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)


# ------------------------------------------------------------------------------------------------ 3. compact packing
def test_third_rows_get_no_gradient_from_the_term(smpl, tables, dev):
    """The term reaches the raw rotations through the Gram-Schmidt backward only: with reg_pose_body 0 the third rows' gradient
    entries are exact zeros."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F = 37
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 111)
    md = markers.to(dev)
    cfg = _cfg(_lists(tables)["builder"], W_CHAMFER, W_MARKER)
    cfg["stages"]["chamfer"]["losses"]["reg_pose_body"] = 0.0
    cfg["stages"]["marker"]["losses"]["reg_pose_body"] = 0.0
    pc = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    assert pc.capsules_on
    x = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    _, g, _ = pc.evaluate(x)
    gp = g[4 * F + 10:].reshape(F, 23, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any()
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, cfg)
    assert pm.capsules_on
    xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    _, g, _ = pm.evaluate(xm)
    gp = g[:207 * F].reshape(F, 23, 3, 3)
    groot = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any() and not groot[:, 2].any()


# ------------------------------------------------------------------------------------------------ 4. fused vs composed
@pytest.mark.parametrize("F", [7, 300])
def test_fused_and_composed_capsule_solves_agree(smpl, tables, dev, F):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.capsule_fused: False): the start agrees to 1e-5, the end to 5e-2 / 8e-2
    (test_fused_and_composed_foot_lock_solves_agree's tolerances), and both decrease.  The builder's capsules with doubled
    radii, weights 10 / 1 (the stages' own data weights: a centimetre of overlap weighs like a centimetre of marker error)."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    M = 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    out = {}
    for fused in (True, False):
        cfg = _cfg(_lists(tables)["builder"], 10.0, 1.0)
        cfg["execution"] = {"capsule_fused": fused}
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
    print("OBS capsules fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
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
    md = markers.to(dev)
    cj, cg, pr = (np.ascontiguousarray(x) for x in _lists(tables)["builder"])
    on = _cfg((cj, cg, pr), W_CHAMFER, W_MARKER)

    def arm(p, w=1.0):  # what no config can produce: the library itself must refuse it
        p.cap_joints, p.cap_geom, p.cap_pairs, p.cap_w = cj, cg, pr, w

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
    # the setter: every bad argument; off with null pointers
    lib, fit = smpl.device_model.lib, pp.fit
    C, P = len(cj), len(pr)

    def call(w=1.0, c=C, j=cj, g=cg, p=P, q=pr):
        j, g, q = (None if a is None else np.ascontiguousarray(a) for a in (j, g, q))
        return lib.uuo_fit_set_capsules(fit, w, c, None if j is None else j.ctypes.data, None if g is None else g.ctypes.data, p,
                                        None if q is None else q.ctypes.data)

    def edit(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b

    assert call() == 0
    for w in (-1.0, float("nan"), float("inf")):
        assert call(w=w) != 0                                                                   # weight
    big_j, big_g = np.tile(cj, (2, 1))[:33], np.tile(cg, (2, 1))[:33]
    assert call(c=0) != 0 and call(c=33, j=big_j, g=big_g) != 0 and call(c=-1) != 0             # C outside 1 .. 32
    assert call(c=32, j=big_j[:32], g=big_g[:32]) == 0 and call(c=2, p=1, q=np.array([[0, 1]], dtype=np.int32)) == 0
    big_p = np.tile(pr, (2, 1))[:257]
    assert call(p=0) != 0 and call(p=257, q=big_p) != 0 and call(p=256, q=big_p[:256]) == 0     # P outside 1 .. 256
    for bad in (24, -1):
        assert call(j=edit(cj, (3, 1), bad)) != 0                                               # a joint id outside [0, 24)
    assert call(j=edit(cj, (3, 1), cj[3, 0])) != 0                                              # u == v
    for bad in (float("nan"), float("inf")):
        assert call(g=edit(cg, (2, 0), bad)) != 0 and call(g=edit(cg, (2, 1), bad)) != 0        # alpha, beta
        assert call(g=edit(cg, (2, 2), bad)) != 0                                               # radius
    assert call(g=edit(cg, (2, 2), 0.0)) != 0 and call(g=edit(cg, (2, 2), -0.1)) != 0           # radius <= 0
    for bad in (C, -1):
        assert call(q=edit(pr, (5, 1), bad)) != 0                                               # a pair index outside [0, C)
    assert call(q=edit(pr, (5, 1), pr[5, 0])) != 0                                              # i == j
    assert call(j=None) != 0 and call(g=None) != 0 and call(q=None) != 0                        # null arrays with w > 0
    assert call(w=0.0, c=0, j=None, g=None, p=0, q=None) == 0                                   # off, null pointers
    assert pp.evaluate(x)[0] == loss0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), on)
    assert p.capsules_on
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step.*self_penetration"):
        solve_batch([p], [xc], max_iter=3)


# ------------------------------------------------------------------------------------------------ 6. what it buys


def _quality(out, seq, oracle_smpl, caps, window):
    """(mean depth in mm of the frames' deepest overlap inside `window`, or over all frames without one; mean vertex error in m
    over all frames)"""
    from uuo_mocap_amd.metrics import compute_self_penetration

    r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
    j = r["joints"][:, :24]
    if window is not None:
        j = j[window[0]:window[1]]
    return (compute_self_penetration(j, *caps)["mean_depth_mm"],
            float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean()))


def test_capsules_config(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic capture (seed 0), the default one and the one whose HMR start has the left arm 30 mm inside the torso
    for 24 frames while the arm's markers are missing (self_penetration=True), fitted with video_mocap.yaml and with
    video_mocap_capsules.yaml.  Required (DESIGN 4o's rule): the window's mean depth at most half the plain fit's, and the mean
    vertex error over all frames at most the plain fit's + 0.5 mm on both captures.  Measured with the shipped 0.1 / 0.01 (the
    sweep's run; fits repeat to a few hundredths of a millimetre): window
    depth 25.6 -> 6.1 mm (0.24 x), vertex error 13.18 -> 11.20 mm there and 6.73 -> 6.92 mm on the default capture (whose random
    ground-truth motion itself overlaps, 8.7 mm on average: there the term can only cost, and a decade more costs 0.9 mm)."""
    caps = body_capsules(tables)
    res = {}
    for tag, kw in (("default", {}), ("penetrating", {"self_penetration": True})):
        seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50, **kw)
        window = seq.gt.get("penetration_window")
        for name in ("video_mocap", "video_mocap_capsules"):
            res[(tag, name)] = _quality(_fit(seq, name, smpl, dev), seq, oracle_smpl, caps, window)
            record_property("%s_%s_depth_mm" % (tag, name), res[(tag, name)][0])
            record_property("%s_%s_vertex_m" % (tag, name), res[(tag, name)][1])
        (d0, v0), (d1, v1) = res[(tag, "video_mocap")], res[(tag, "video_mocap_capsules")]
        print("OBS capsules (%s capture): mean depth plain %.3f capsules %.3f mm; vertex error plain %.2f capsules %.2f mm"
              % (tag, d0, d1, 1e3 * v0, 1e3 * v1))
    d0, _ = res[("penetrating", "video_mocap")]
    assert d0 >= 1.0, "the capture does not show the failure: %r" % (res,)
    assert res[("penetrating", "video_mocap_capsules")][0] <= 0.5 * d0, res
    for tag in ("default", "penetrating"):
        assert res[(tag, "video_mocap_capsules")][1] <= res[(tag, "video_mocap")][1] + 5e-4, (tag, res)
