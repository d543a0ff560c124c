"""The root stage's fused closure (UUO_STAGE_ROOT: a yaw per frame, UUO_STAGE_ROOT_SHARED: one yaw) on the device: against the
float64 restatement (root_ref64) at the assignment the kernel reports, the reported winners as float64 minimisers, the shared
packing against a PartProblem on all vertices, bit-reproducibility, the solve against torch's L-BFGS in float64, and the
pipeline on video_mocap_root.yaml."""
import copy

import numpy as np
import pytest
import torch

from gpu_support import _check_grad, _inputs, dev, smpl, smpl64  # noqa: F401  (fixtures)
from root_ref64 import ref_root64, root_vertices64
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence

pytestmark = pytest.mark.gpu

# trans_vel where it has to show: the data term's gradient on a translation entry is about 2 w_fc |mean residual| / F =
# 20 x 0.025 / F = 0.5 / F at _inputs' perturbations (2 cm on the translation, markers 1-2 cm off their vertices); trans_vel's is
# 2 w_tv (r_{t-1} - r_t) / (3 (F - 1)) with r the 2 cm translation noise differenced twice, about 0.05: 0.033 w_tv / (F - 1).
# A tenth of the data term's needs w_tv >= 1.5; 10 leaves a factor of six (and a missing frame, whose marker mean is the origin,
# only adds to it).  The test asserts the ratio on the float64 gradients.
W_TVEL = 10.0


def _cfg(shared, tvel=0.0, **root):
    cfg = copy.deepcopy(packaged_config("video_mocap_root"))
    st = cfg["stages"]["root"]
    st.update(yaw_lock=not shared, constrained_rotation=shared)
    if tvel:
        st["losses"]["trans_vel"] = tvel
    st.update(root)
    return cfg


def _blocks(F, shared):
    nz = 1 if shared else F
    return (("trans", slice(0, 3 * F)), ("z", slice(3 * F, 3 * F + nz)), ("betas", slice(3 * F + nz, None)))


def _present(markers, trans):
    """every entry present: the capture's missing entries (exact zeros) replaced by a point 10 cm off the frame's median"""
    out = markers.clone()
    gone = out.abs().sum(-1) == 0
    out[gone] = (trans[:, None, :] + 0.1).expand_as(out)[gone]
    return out


def _case(tables, F, M, seed, holes=True):
    """_inputs' capture and perturbed point with every entry present, then (holes) column 0 missing throughout where there is
    another column and frame 1 entirely missing where there is another frame: sum mask != F M.  (At M = 1 or F = 1 the
    deletion would leave no marker at all: that is test_every_marker_missing's case.)"""
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, F, seed, M)
    markers = _present(markers, trans)
    if holes and M >= 2:
        markers[:, 0] = 0.0
    if holes and F >= 2:
        markers[1] = 0.0
    return markers, o_pose, o_betas, root, pert


def _problem(smpl, dev, cfg, markers, o_pose, o_betas, root):  # noqa: F811
    from uuo_mocap_amd.engine import RootProblem

    return RootProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)


def _pack(prob, pert, dev):  # noqa: F811
    tp, zp, bp, pp, rp = pert
    return prob.pack(tp.to(dev), (zp[:1] if prob.shared else zp).to(dev), bp.to(dev))


# ------------------------------------------------------------------------------------------------ 1. closure against float64
@pytest.mark.parametrize("tvel", [0.0, W_TVEL])
@pytest.mark.parametrize("M", [1, 16, 17, 50])
@pytest.mark.parametrize("F", [1, 2, 3, 33])
@pytest.mark.parametrize("shared", [False, True])
def test_closure_against_float64(smpl, smpl64, tables, dev, record_property, shared, F, M, tvel):  # noqa: F811
    """Loss within 2e-5 and gradient within gpu_support._check_grad of the float64 restatement at the reported assignment.  F:
    no velocity pair, one pair, the first interior frame, more frames than the finalisation has groups; M: both sides of the
    one-wave / fused-forward boundary (16 | 17)."""
    _closure_against_float64(smpl, smpl64, tables, dev, record_property, shared, F, M, tvel)


def _closure_against_float64(smpl, smpl64, tables, dev, record_property, shared, F, M, tvel):  # noqa: F811
    markers, o_pose, o_betas, root, pert = _case(tables, F, M, 1000 + 10 * F + M)
    mask_sum = int((markers.abs().sum(-1) != 0).sum())
    assert 0 < mask_sum and (mask_sum != F * M or (M == 1 and F == 1))
    cfg = _cfg(shared, tvel)
    prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, root)
    assert prob.n == (3 * F + 11 if shared else 4 * F + 10)
    x = _pack(prob, pert, dev)
    loss, grad, nn = prob.evaluate(x)
    assert nn.min() >= 0 and nn.max() < 6890
    lo, g_ref = ref_root64(smpl64, cfg, markers, o_pose, o_betas, root, x, nn, shared)
    name = "root_%s_F%d_M%d_tv%g" % ("shared" if shared else "frame", F, M, tvel)
    record_property("loss_rel_%s" % name, abs(loss - lo) / abs(lo))
    print("%s loss %.8g ref %.8g" % (name, loss, lo))
    if tvel and F >= 2:   # the weight does what the note above says, judged on the float64 gradients alone
        _, g_plain = ref_root64(smpl64, _cfg(shared), markers, o_pose, o_betas, root, x, nn, shared)
        ratio = np.linalg.norm((g_ref - g_plain)[:3 * F]) / np.linalg.norm(g_plain[:3 * F])
        record_property("tvel_share_%s" % name, float(ratio))
        assert ratio >= 0.1, (name, ratio)
    np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
    _check_grad(grad.cpu().numpy(), g_ref, _blocks(F, shared), name, record_property)


@pytest.mark.parametrize("shared", [False, True])
def test_finalisation_loops_past_their_first_round(smpl, smpl64, tables, dev, record_property, shared):  # noqa: F811
    """test_closure_against_float64's asserts at F = 1025, M = 17 with trans_vel on: every loop of k_finalize_root takes a second
    round there -- the partial sums stride 256 frames, the translation's entries 1024 (3 F > 1024), the per-frame yaw's 1024
    frames (F > 1024)."""
    _closure_against_float64(smpl, smpl64, tables, dev, record_property, shared, 1025, 17, W_TVEL)


@pytest.mark.parametrize("shared", [False, True])
def test_every_marker_missing(smpl, smpl64, tables, dev, shared):  # noqa: F811
    """No marker present: the loss is the two priors alone and the gradient is finite (the data term's share is exact zeros)."""
    F, M = 3, 17
    markers, o_pose, o_betas, root, pert = _case(tables, F, M, 77, holes=False)
    markers = torch.zeros_like(markers)
    cfg = _cfg(shared, W_TVEL)
    prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, root)
    x = _pack(prob, pert, dev)
    loss, grad, nn = prob.evaluate(x)
    tp, zp, bp = pert[:3]
    mm = markers.double().mean(1)
    priors = 0.1 * float(((bp.double() - o_betas.double()) ** 2).mean()) + \
        W_TVEL * float((((tp.double()[1:] - tp.double()[:-1]) - (mm[1:] - mm[:-1])) ** 2).mean())
    np.testing.assert_allclose(loss, priors, rtol=2e-5)
    g = grad.cpu().numpy()
    assert np.isfinite(g).all()
    nz = 1 if shared else F
    assert not g[3 * F:3 * F + nz].any()   # nothing reads the yaw
    lo, g_ref = ref_root64(smpl64, cfg, markers, o_pose, o_betas, root, x, nn.clamp(0, 6889), shared)
    np.testing.assert_allclose(g, g_ref, rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 2. the winners
@pytest.mark.parametrize("M", [16, 17, 50])
@pytest.mark.parametrize("shared", [False, True])
def test_reported_winners_are_float64_minimisers(smpl, smpl64, tables, dev, record_property, shared, M):  # noqa: F811
    """For every present entry d2_64[nn] - min_v d2_64 <= 1e-5 m^2: fp32 rounding of |x|^2 - 2 x.v + |v|^2 at 2 m from the origin is
    about 5e-7, an fp32 skinning error of 1e-6 m at distances up to 1 m adds 2e-6."""
    F = 3
    markers, o_pose, o_betas, root, pert = _case(tables, F, M, 2000 + M)
    prob = _problem(smpl, dev, _cfg(shared), markers, o_pose, o_betas, root)
    x = _pack(prob, pert, dev)
    _, _, nn = prob.evaluate(x)
    v = root_vertices64(smpl64, o_pose, root, x, shared)                           # [F, V, 3]
    d2 = ((markers.double().numpy()[:, :, None, :] - v[:, None, :, :]) ** 2).sum(-1)  # [F, M, V]
    won = np.take_along_axis(d2, nn.cpu().numpy().astype(np.int64)[..., None], axis=2)[..., 0]
    excess = (won - d2.min(axis=2))[(markers.abs().sum(-1) != 0).numpy()]
    record_property("winner_excess_%s_M%d" % ("shared" if shared else "frame", M), float(excess.max()))
    print("largest excess over the float64 minimum: %.3e m^2" % excess.max())
    assert excess.size and excess.max() <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. against the part stage
@pytest.mark.parametrize("M", [16, 17])
def test_shared_packing_agrees_with_a_part_problem_on_all_vertices(smpl, tables, dev, record_property, M):  # noqa: F811
    """All markers present, trans_vel off: UUO_STAGE_ROOT_SHARED is the part stage's closure on vertex_indices = arange(6890)
    at the same weights ([z | trans | betas] there, [trans | z | betas] here)."""
    from uuo_mocap_amd.engine import PartProblem

    F = 5
    markers, o_pose, o_betas, root, pert = _case(tables, F, M, 3000 + M, holes=False)
    part_cfg = packaged_config("hmr_part")
    w = part_cfg["stages"]["part"]["losses"]
    cfg = _cfg(True)
    cfg["stages"]["root"]["losses"] = {"full_chamfer": float(w["chamfer"]), "reg_betas": float(w["reg_betas"])}
    prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, root)
    x = _pack(prob, pert, dev)
    loss, grad, nn = prob.evaluate(x)
    part = PartProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), torch.arange(6890), part_cfg)
    tr, z, b = prob.unpack(x)
    loss_p, grad_p, nn_p = part.evaluate(part.pack(z, tr, b))
    gz, gt, gb = part.unpack(grad_p)
    g_part = torch.cat([gt.reshape(-1), gz.reshape(-1), gb.reshape(-1)])
    same = loss == loss_p and torch.equal(grad, g_part) and torch.equal(nn, nn_p)
    record_property("bit_identical_to_part_M%d" % M, bool(same))
    print("root (shared) against part on all vertices, M = %d: bit-identical %s; loss %.8g / %.8g" % (M, same, loss, loss_p))
    assert same
    assert torch.equal(nn, nn_p)
    np.testing.assert_allclose(loss, loss_p, rtol=2e-5)
    _check_grad(grad.cpu().numpy(), g_part.cpu().numpy().astype(np.float64), _blocks(F, True), "root_vs_part_M%d" % M,
                record_property)


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("M", [16, 50])
def test_bit_reproducible_also_with_the_other_packing_in_between(smpl, tables, dev, M):  # noqa: F811
    F = 33
    markers, o_pose, o_betas, root, pert = _case(tables, F, M, 4000 + M)
    for shared in (False, True):
        prob = _problem(smpl, dev, _cfg(shared, W_TVEL), markers, o_pose, o_betas, root)
        other = _problem(smpl, dev, _cfg(not shared, 0.5 * W_TVEL), markers, o_pose, o_betas, root)
        assert prob.fit == other.fit   # the same workspace
        x, xo = _pack(prob, pert, dev), _pack(other, pert, dev) + 0.01
        l1, g1, n1 = prob.evaluate(x)
        l2, g2, n2 = prob.evaluate(x)
        assert l1 == l2 and torch.equal(g1, g2) and torch.equal(n1, n2)
        other.evaluate(xo)
        l3, g3, n3 = prob.evaluate(x)
        assert l1 == l3 and torch.equal(g1, g3) and torch.equal(n1, n3)


# ------------------------------------------------------------------------------------------------ 5. the solve
def _torch_lbfgs64(smpl64, cfg, markers, o_pose, o_betas, root, x0, shared, lr, max_iter):  # noqa: F811
    """torch.optim.LBFGS(strong_wolfe, history 100) in float64 on the restated closure, the brute-force argmin redone at every
    evaluation: (final loss = the last loss the optimiser accepted, evaluations)"""
    x = x0.detach().cpu().double().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([x], lr=lr, max_iter=max_iter, history_size=100, tolerance_grad=cfg["optimizer"]["tolerance_grad"],
                            tolerance_change=cfg["optimizer"]["tolerance_change"], line_search_fn="strong_wolfe")
    md = markers.double().numpy()
    evals = [0]

    def closure():
        opt.zero_grad()
        v = root_vertices64(smpl64, o_pose, root, x, shared)
        d2 = ((md[:, :, None, :] - v[:, None, :, :]) ** 2).sum(-1)
        nn = torch.from_numpy(d2.argmin(axis=2))
        loss, grad = ref_root64(smpl64, cfg, markers, o_pose, o_betas, root, x, nn, shared)
        x.grad = torch.from_numpy(grad).reshape(x.shape)
        evals[0] += 1
        return torch.tensor(loss, dtype=torch.float64)

    opt.step(closure)
    v = root_vertices64(smpl64, o_pose, root, x, shared)
    nn = torch.from_numpy(((md[:, :, None, :] - v[:, None, :, :]) ** 2).sum(-1).argmin(axis=2))
    return ref_root64(smpl64, cfg, markers, o_pose, o_betas, root, x, nn, shared)[0], evals[0]


@pytest.mark.parametrize("shared", [False, True])
def test_solve_against_float64_lbfgs(smpl, smpl64, tables, dev, record_property, shared):  # noqa: F811
    """F = 8, M = 20 from a translation 0.3 m off and an input root yawed by -0.4 rad, 50 iterations: the loss falls, ends within
    5 % of torch's float64 L-BFGS on the restated closure (the band of tests/test_gpu_parity.py's marker-stage solve), the
    in-place contract of reference optimization.py:136-144 holds and iter_fn is called once per evaluation."""
    from uuo_mocap_amd.optimization import LAST_STATS, optim_root
    from uuo_mocap_amd.transforms import compute_root_orient_z

    F, M = 8, 20
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 51, M)
    markers = _present(markers, trans)
    cfg = _cfg(shared, num_iters=50)
    trans0 = torch.from_numpy(np.asarray(seq.gt["trans"])).float() + 0.3
    root_in = (compute_root_orient_z(torch.full((F, 1, 1), -0.4)) @ root).contiguous()
    betas0 = o_betas.clone()
    calls = []
    d_trans, d_betas, d_root = trans0.clone().to(dev), betas0.clone().to(dev), root_in.clone().to(dev).requires_grad_(True)
    optim_root(markers.to(dev), o_pose.to(dev), d_betas, d_root, d_trans, None, smpl, cfg,
               iter_fn=lambda **kw: calls.append(kw))
    st = LAST_STATS["root"]
    assert st["final_loss"] < st["first_loss"], st
    # the in-place contract: trans / betas are the solved leaves, root_orient = Rz(z) @ its input
    assert not torch.equal(d_trans.cpu(), trans0) and d_root.requires_grad
    last = [c for c in calls if c["iteration"] == len(calls) - 1][0]
    assert [c["stage"] for c in calls] == ["root"] * len(calls) and len(calls) == st["n_eval"]
    assert [c["iteration"] for c in calls] == list(range(len(calls)))
    assert set(last) == {"stage", "iteration", "pose_body", "betas", "trans", "root_orient"}
    assert last["trans"].shape == (F, 3) and last["betas"].shape == (1, 10) and last["root_orient"].shape == (F, 1, 3, 3)
    # z from the rotation applied: R_out = Rz(z) R_in  =>  Rz = R_out R_in^T, a pure yaw, one angle for the shared packing
    rz = (d_root.detach().cpu() @ root_in.transpose(-1, -2))[:, 0].double()
    zed = torch.atan2(rz[:, 1, 0], rz[:, 0, 0])
    back = compute_root_orient_z(zed.float().reshape(F, 1, 1)) @ root_in
    np.testing.assert_allclose(d_root.detach().cpu().numpy(), back.numpy(), atol=2e-6)
    if shared:
        assert float(zed.max() - zed.min()) < 1e-6
    # the solved leaves give the reported final loss
    from uuo_mocap_amd.engine import RootProblem
    probe = RootProblem(smpl, markers.to(dev), o_pose.to(dev), betas0.to(dev), d_root.detach(), cfg)
    l_end, _, _ = probe.evaluate(probe.pack(d_trans, torch.zeros(probe.nz, 1, 1, device=dev), d_betas))
    np.testing.assert_allclose(l_end, st["final_loss"], rtol=1e-4)
    x0 = torch.cat([trans0.reshape(-1), torch.zeros(1 if shared else F), betas0.reshape(-1)])
    ref_final, ref_evals = _torch_lbfgs64(smpl64, cfg, markers, o_pose, betas0, root_in, x0, shared, 0.1, 50)
    for k, v in (("final", st["final_loss"]), ("first", st["first_loss"]), ("evals", st["n_eval"]), ("ref_final", ref_final),
                 ("ref_evals", ref_evals)):
        record_property("root_solve_%s_%s" % ("shared" if shared else "frame", k), float(v))
    print("root solve (%s): first %.6g final %.6g in %d evaluations; float64 torch L-BFGS final %.6g in %d evaluations"
          % ("shared" if shared else "frame", st["first_loss"], st["final_loss"], st["n_eval"], ref_final, ref_evals))
    assert abs(st["final_loss"] - ref_final) <= 0.05 * ref_final, (st["final_loss"], ref_final)


# ------------------------------------------------------------------------------------------------ 6. the pipeline
def test_pipeline_runs_the_root_stage(smpl, tables, dev):  # noqa: F811
    """multimodal_video_mocap on video_mocap_root.yaml cut to F = 12, M = 20 with the stages' iterations lowered."""
    from uuo_mocap_amd.multimodal import last_run_stats, multimodal_video_mocap

    F, M = 12, 20
    seq = make_sequence(tables, seed=9, num_frames=F, num_markers=M)
    cfg = packaged_config("video_mocap_root")
    for k, n in (("root", 30), ("chamfer", 5), ("marker", 5)):
        cfg["stages"][k]["num_iters"] = n
    out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0),
                                 dev, cfg, offset=0, print_options=[], save_stages=True, smpl_inference=smpl)
    stats = last_run_stats()
    assert stats["root"]["final_loss"] < stats["root"]["first_loss"], stats["root"]
    assert "root" in [label for label, _ in stats["timeline"]]
    rec = out["stages"]["root"]
    assert set(rec) == {"trans", "root_orient", "betas", "pose_body"}
    assert rec["trans"].shape == (F, 3) and rec["root_orient"].shape == (F, 1, 3, 3) and rec["betas"].shape == (10,)
    assert rec["pose_body"].shape == (F, 23, 3, 3)
    assert out["trans"].shape == (F, 3) and torch.isfinite(out["trans"]).all()
