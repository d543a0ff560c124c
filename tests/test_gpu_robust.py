"""EXTENSION: Geman-McClure (GMoF) data terms on the fused closures (uuo_problem_t.robust_sigma) on the MI355X -- every stage
closure against float64 autograd through the oracle's SMPL, the sigma limits, lock-step batches, the operator-composed route
and a fit on a capture with ghost markers."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_support import _rel_err, _three_corners, dev, smpl, smpl64  # noqa: E402,F401
from stage_ref64 import ref_chamfer64, ref_marker64, ref_part64  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 50


# the stage references at the sigma of the call (this file passes it next to the config)
def _ref_chamfer(smpl64, cfg, sigma, *args):
    return ref_chamfer64(smpl64, cfg, *args, sigma=sigma)


def _ref_marker(smpl64, cfg, sigma, *args):
    return ref_marker64(smpl64, None, cfg, *args, sigma=sigma)


def _ref_part(smpl64, cfg, sigma, *args):
    return ref_part64(smpl64, cfg, *args, sigma=sigma)


def _ghosts(markers, frac, seed, columns=()):
    """A copy of `markers` [F, M, 3] with about `frac` of its present (frame, marker) entries and the whole `columns` moved
    0.3 - 1.0 m away in random directions (ghost points of an unlabeled capture)."""
    gen = torch.Generator().manual_seed(seed)
    out = markers.clone()
    F_, M_ = out.shape[:2]
    hit = torch.rand(F_, M_, generator=gen) < frac
    for c in columns:
        hit[:, c] = True
    hit &= out.abs().sum(-1) != 0
    d = torch.randn(F_, M_, 3, generator=gen)
    d = d / d.norm(dim=-1, keepdim=True) * (0.3 + 0.7 * torch.rand(F_, M_, 1, generator=gen))
    out[hit] = out[hit] + d[hit]
    return out


def _inputs(tables, F, seed):
    seq = make_sequence(tables, seed=seed, num_frames=F, num_markers=M)
    markers = _ghosts(torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float(), 0.05, seed + 1, columns=(3,))
    o_pose = seq.img_smpl.pose_body.clone().float()
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float()
    root = seq.img_smpl.root_orient.clone().float()
    trans = torch.median(markers, dim=1)[0].clone()
    gen = torch.Generator().manual_seed(seed + 2)
    r = lambda *s: torch.randn(*s, generator=gen)
    pert = (trans + 0.02 * r(F, 3), 0.3 * r(F, 1, 1), o_betas + 0.3 * r(1, 10), o_pose + 0.05 * r(F, 23, 3, 3),
            root + 0.05 * r(F, 1, 3, 3))
    return seq, markers, o_pose, o_betas, root, trans, pert


def _cfg(sigma, name="video_mocap"):
    cfg = packaged_config(name)
    for k in ("chamfer", "part", "marker"):
        cfg["stages"][k]["robust_sigma"] = sigma
    return cfg


def _leg_vertices(smpl, dev):
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    return torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("F", [1, 37, 300])
@pytest.mark.parametrize("sigma", [0.01, 0.05])
def test_robust_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, sigma):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 40 + F)
    cfg, cfg0 = _cfg(sigma), _cfg(0.0)
    md = markers.to(dev)

    # chamfer stage
    prob = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    prob0 = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg0)
    assert prob.problem.robust_sigma == pytest.approx(sigma)
    x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    loss, grad, nn = prob.evaluate(x)
    _, _, nn0 = prob0.evaluate(x)
    assert torch.equal(nn, nn0), "rho is monotone: the assignment must not change"
    lo, g_ref = _ref_chamfer(smpl64, cfg, sigma, markers, o_pose, o_betas, root, x, nn)
    np.testing.assert_allclose(loss, lo, rtol=2e-5)
    assert _rel_err(grad.cpu().numpy(), g_ref) < 2e-4

    # part stage: 50 markers on a leg (four-wave kernel) and the first ten of them (one-wave kernel)
    vidx = _leg_vertices(smpl, dev)
    for mk in (M, 10):
        mm = md[:, :mk].contiguous()
        pp_ = PartProblem(smpl, mm, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, cfg)
        pp0 = PartProblem(smpl, mm, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, cfg0)
        xp = pp_.pack(torch.full((1, 1, 1), 0.2, device=dev), tp.to(dev), bp.to(dev))
        for k in range(2):  # the second evaluation runs on the pose-blend cache the first one built
            lp, gp, nnp = pp_.evaluate(xp)
            _, _, nnp0 = pp0.evaluate(xp)
            assert torch.equal(nnp, nnp0)
            lo, g_ref = _ref_part(smpl64, cfg, sigma, markers[:, :mk], o_pose, o_betas, root, xp, vidx, nnp)
            np.testing.assert_allclose(lp, lo, rtol=2e-5)
            assert _rel_err(gp.cpu().numpy(), g_ref) < 2e-4, (mk, k)
            xp = xp * 0.97 + 0.01

    # marker stage: one-hot placement and three-corner placement
    xm = None
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F)
    for assign, bary in ((vids, None), (i3, b3)):
        pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), assign.to(dev), cfg,
                           bary=None if bary is None else bary.to(dev))
        if xm is None:
            xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        lm, gm, _ = pm.evaluate(xm)
        lo, g_ref = _ref_marker(smpl64, cfg, sigma, markers, o_pose, o_betas, xm, assign, bary)
        np.testing.assert_allclose(lm, lo, rtol=2e-5)
        assert _rel_err(gm.cpu().numpy(), g_ref) < 2e-4, "three-corner" if bary is not None else "one-hot"


# ------------------------------------------------------------------------------------------------ 2. limits
def test_sigma_limits(smpl, tables, dev):
    """sigma = 1e3 m is the square to fp32 rounding; sigma = 0 is bit for bit a config without the key."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem

    F = 37
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 7)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(dev)
    i3, b3 = _three_corners(tables, seq, 3)
    vidx = _leg_vertices(smpl, dev)
    absent = packaged_config("video_mocap")
    for k in ("chamfer", "part", "marker"):
        assert "robust_sigma" not in absent["stages"][k]
    makers = {
        "chamfer": (lambda c: ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), c),
                    lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))),
        "part": (lambda c: PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, c),
                 lambda p: p.pack(torch.full((1, 1, 1), 0.2, device=dev), tp.to(dev), bp.to(dev))),
        "marker": (lambda c: MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, c),
                   lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
        "marker3": (lambda c: MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), i3.to(dev), c, bary=b3.to(dev)),
                    lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
    }
    for name, (make, pack) in makers.items():
        pa, p0, pbig = make(absent), make(_cfg(0.0)), make(_cfg(1e3))
        x = pack(pa)
        la, ga, na = pa.evaluate(x)
        l0, g0, n0 = p0.evaluate(x)
        lb, gb, nb = pbig.evaluate(x)
        assert la == l0 and torch.equal(ga, g0), name
        assert (na is None and n0 is None) or torch.equal(na, n0)
        assert lb == pytest.approx(la, rel=1e-6), name
        assert _rel_err(gb.cpu().numpy(), ga.cpu().numpy()) < 1e-5, name


# ------------------------------------------------------------------------------------------------ 3. lock-step batches
def test_robust_lockstep_batch_is_bit_identical_to_solving_one_by_one(smpl, dev):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem, solve_batch
    from uuo_mocap_amd.transforms import compute_root_orient_z

    F, Mk = 21, 9
    seq = make_sequence(smpl.tables, seed=31, num_frames=F, num_markers=Mk)
    markers = _ghosts(torch.from_numpy(seq.markers.get_points()).float(), 0.05, 5).to(dev)
    cfg = _cfg(0.05)
    o_pose = seq.img_smpl.pose_body.to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).to(dev)
    root = seq.img_smpl.root_orient.to(dev)
    trans = torch.median(markers, dim=1)[0]
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)

    def check(make_problems, make_x, max_iter, lr):
        probs_a, probs_b = make_problems(), make_problems()
        assert all(p.problem.robust_sigma > 0 for p in probs_a)
        xs_a = [make_x(p, i) for i, p in enumerate(probs_a)]
        xs_b = [x.clone() for x in xs_a]
        alone = [p.solve(x, max_iter=max_iter, lr=lr) for p, x in zip(probs_a, xs_a)]
        together = solve_batch(probs_b, xs_b, max_iter=max_iter, lr=lr)
        for i, (sa, sb, xa, xb) in enumerate(zip(alone, together, xs_a, xs_b)):
            assert (sa["n_iter"], sa["n_eval"], sa["stop_reason"]) == (sb["n_iter"], sb["n_eval"], sb["stop_reason"]), (i, sa, sb)
            assert sa["first_loss"] == sb["first_loss"] and sa["final_loss"] == sb["final_loss"], (i, sa, sb)
            assert torch.equal(xa, xb), "problem %d: iterates differ" % i

    def chamfer_problems():  # the four yaw hypotheses of multimodal_video_mocap
        return [ChamferProblem(smpl, markers, o_pose, o_betas,
                               (compute_root_orient_z(torch.full((F, 1, 1), k * np.pi / 2, device=dev)) @ root).contiguous(), cfg)
                for k in range(4)]

    check(chamfer_problems, lambda p, i: p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose), max_iter=25, lr=0.1)

    def marker_problems():
        return [MarkerProblem(smpl, markers, o_pose, o_betas, torch.randperm(6890, generator=torch.Generator().manual_seed(k))[:Mk]
                              .to(torch.int32).to(dev), cfg) for k in range(3)]

    check(marker_problems, lambda p, i: p.pack(o_pose, o_betas, root, trans), max_iter=20, lr=1.0)

    subtrees = [[0, 1, 4, 7, 10], [0, 2, 5, 8, 11], [3, 6, 9, 12, 15], [9, 13, 16, 18, 20]]

    def part_problems():
        ps = [PartProblem(smpl, markers, o_pose, o_betas, root,
                          torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in st_]), cfg) for st_ in subtrees]
        for p in ps[1:]:
            p.problem.pose_cache_id = ps[0].problem.pose_cache_id
        return ps

    check(part_problems, lambda p, i: p.pack(torch.zeros(1, 1, 1, device=dev), trans, o_betas), max_iter=40, lr=1.0)


# ------------------------------------------------------------------------------------------------ 4. fused vs composed
def test_fused_and_composed_robust_solves_agree(smpl, tables, dev):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closure and on the operator-composed one
    (execution.robust_fused: False): the start must agree to 1e-5 and the end to the tolerances of
    test_chamfer_stage_options_match_reference."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    F = 37
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 21)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    out = {}
    for fused in (True, False):
        cfg = _cfg(0.05)
        cfg["execution"] = {"robust_fused": fused}
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 25
        pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
        optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                      trans=tr, img_mask=torch.ones(F, device=dev), marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev),
                      smpl_inference=smpl, config=cfg)
        sc = dict(last_stats("chamfer"))
        o_pose_m = pose.detach().clone()
        optim_markers(md, pose_body=pose, o_pose_body=o_pose_m, betas=betas, o_betas=o_betas.to(dev), root_orient=rt, trans=tr,
                      barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev), smpl_inference=smpl, config=cfg)
        sm = dict(last_stats("marker"))
        out[fused] = (sc, sm, tr.detach().cpu().clone())
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    (cf, mf, _), (cc, mc, _) = out[True], out[False]
    assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
    print("OBS robust fused vs composed: chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=8e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)


# ------------------------------------------------------------------------------------------------ 5. ghost markers
def _fit_error(seq, points, cfg_name, smpl, oracle_smpl, dev):
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(points.copy(), 30.0), dev,
                                 packaged_config(cfg_name), offset=0, print_options=[], save_stages=False,
                                 smpl_inference=smpl)
    v = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())["vertices"]
    gt = torch.from_numpy(seq.gt["verts"])
    return float((v - gt).norm(dim=-1).mean())


def test_ghost_markers_robust_config_recovers_the_body(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic sequence; 5 % of the (frame, marker) entries and two whole columns replaced by points 0.3 - 1.0 m
    from the body.  video_mocap_robust.yaml must fit the body clearly closer to the ground truth than video_mocap.yaml, and
    cost at most 0.5 mm on the clean sequence.  Measured figures: DESIGN.md section 4l."""
    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=M)
    clean = np.asarray(seq.markers.get_points()).copy()
    ghost = _ghosts(torch.from_numpy(np.nan_to_num(clean)).float(), 0.05, 77, columns=(11, 29)).numpy()
    ghost[np.isnan(clean)] = np.nan
    errs = {}
    for tag, pts in (("ghost", ghost), ("clean", clean)):
        for name in ("video_mocap", "video_mocap_robust"):
            errs[(tag, name)] = _fit_error(seq, pts, name, smpl, oracle_smpl, dev)
            record_property("v2v_%s_%s_m" % (tag, name), errs[(tag, name)])
    print("OBS ghost markers: mean vertex error plain %.2f mm robust %.2f mm; clean plain %.2f mm robust %.2f mm"
          % tuple(1e3 * errs[k] for k in (("ghost", "video_mocap"), ("ghost", "video_mocap_robust"),
                                           ("clean", "video_mocap"), ("clean", "video_mocap_robust"))))
    # measured (sigma 0.1 m): ghosts 428.75 mm plain, 7.61 mm robust; clean 6.73 mm plain, 6.72 mm robust
    assert errs[("ghost", "video_mocap_robust")] < 0.1 * errs[("ghost", "video_mocap")], errs
    assert errs[("ghost", "video_mocap_robust")] < 1.5e-2, errs
    assert errs[("clean", "video_mocap_robust")] <= errs[("clean", "video_mocap")] + 5e-4, errs
