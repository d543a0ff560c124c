"""EXTENSION: the pose-acceleration term on the local body rotations (stages.{chamfer,marker}.losses.pose_accel,
losses.pose_accel_loss) on the MI355X.  The term has no fused closure: optim_chamfer and optim_markers run it on the closures
composed from the HIP operators.  Checked here: the composed solves' first loss against the plain composed closure plus the
float64 term, that they decrease and smooth the pose, the refusals on a device, and video_mocap_rotsmooth.yaml on the default
capture."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pose_accel_ref64 import pose_accel64  # noqa: E402
from gpu_support import _fit, _inputs, dev, smpl  # noqa: E402,F401
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.metrics import LEAF_JOINT_ROWS  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

U_TABLE = [1.0] * 23
U_TABLE[3], U_TABLE[9], U_TABLE[17] = 0.0, 0.5, 1.75


def _solve_both(smpl, tables, dev, F, cfg):
    """optim_chamfer, then optim_markers from its result, on `cfg`; returns the two statistics records, the start pose and the
    marker stage's start and end pose"""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    Mk = 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(Mk, smpl.device_model.V, device=dev)
    one_hot[torch.arange(Mk), vids.to(dev)] = 1.0
    pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
    optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                  root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                  marker_labels=torch.zeros(F, Mk, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg)
    sc = dict(last_stats("chamfer"))
    mid = pose.detach().cpu().clone()
    optim_markers(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                  trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                  smpl_inference=smpl, config=cfg)
    return sc, dict(last_stats("marker")), o_pose, mid, pose.detach().cpu().clone()


@pytest.mark.parametrize("F", [3, 7])
def test_composed_solves_carry_the_term(smpl, tables, dev, F):
    """25 iterations of both stages at pose_accel 10 / 10 with a joint-weight table, on the composed closures (the term's only
    route: the statistics are the composed driver's).  The chamfer solve's first loss is the plain composed closure's
    (execution.temporal_fused: False, no key: the same operators and driver at the same start) plus the float64 term at the start
    pose, rtol 2e-5 (the project's loss tolerance); the marker solve's likewise at the pose it starts from.  Both decrease, and
    the term itself ends below its start value."""
    def cfg(w):
        c = packaged_config("video_mocap")
        c["execution"] = dict(c.get("execution") or {}, temporal_fused=False)
        for k in ("chamfer", "marker"):
            c["stages"][k]["num_iters"] = 25
            c["stages"][k]["losses"]["joint_accel"] = 1e-12   # (arms execution.temporal_fused: the plain run is composed too)
            if w:
                c["stages"][k]["losses"]["pose_accel"] = w
                c["stages"][k]["pose_accel"] = {"joint_weights": U_TABLE}
        return c

    sc, sm, o_pose, mid, end = _solve_both(smpl, tables, dev, F, cfg(10.0))
    pc, pm, _, pmid, _ = _solve_both(smpl, tables, dev, F, cfg(0.0))
    assert "loss_first" in sc and "loss_first" in sm and "loss_first" in pc and "loss_first" in pm   # composed statistics
    t0 = float(pose_accel64(o_pose.double(), 10.0, U_TABLE))
    print("OBS pose accel composed (F %d): chamfer %.6e -> %.6e (plain first %.6e, term %.6e); marker %.6e -> %.6e"
          % (F, sc["loss_first"], sc["loss_final"], pc["loss_first"], t0, sm["loss_first"], sm["loss_final"]))
    assert t0 > 0.0
    np.testing.assert_allclose(sc["loss_first"], pc["loss_first"] + t0, rtol=2e-5)
    assert sc["loss_final"] < sc["loss_first"] and sm["loss_final"] < sm["loss_first"]
    assert float(pose_accel64(end.double(), 10.0, U_TABLE)) < t0


def test_stage_problems_and_routes_refuse_the_term_where_it_is_not_built(smpl, tables, dev):
    """The fused stage problems refuse a non-zero weight (there is no fused closure), weight 0 evaluates bit for bit as the key
    absent, and frame sharding refuses the key."""
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.engine import ChamferProblem
    from uuo_mocap_amd.optimization import optim_chamfer

    F, Mk = 9, 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103)
    md = markers.to(dev)
    args = (smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev))
    on, zero = packaged_config("video_mocap"), packaged_config("video_mocap")
    on["stages"]["chamfer"]["losses"]["pose_accel"] = 1.0
    zero["stages"]["chamfer"]["losses"]["pose_accel"] = 0.0
    with pytest.raises(NotImplementedError, match="pose_accel.*no fused closure"):
        ChamferProblem(*args, on)
    p0, pz = ChamferProblem(*args, packaged_config("video_mocap")), ChamferProblem(*args, zero)
    x = p0.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    l0, g0, _ = p0.evaluate(x, want_nn=False)
    lz, gz, _ = pz.evaluate(x, want_nn=False)
    assert l0 == lz and torch.equal(g0, gz)
    pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="pose_accel.*frame-block sharding"):
            optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, img_mask=torch.ones(F, device=dev), marker_labels=torch.zeros(F, Mk, dtype=torch.long, device=dev),
                          smpl_inference=smpl, config=on)


def test_rotsmooth_config(smpl, oracle_smpl, tables, dev, record_property):
    """Default 300 x 50 synthetic capture (seed 0), fitted with video_mocap.yaml and with video_mocap_rotsmooth.yaml: the
    rotation-acceleration errors over the leaf joints (10, 11, 15, 22, 23) and over all 23 body joints and the mean vertex error
    are reported (record_property); required: the leaf-joint error of the new config is lower than the plain config's, and its
    vertex error is within 0.5 mm of the plain config's.  Measured with the shipped 1000 / 1000: leaf 458.8 -> 0.126,
    all joints 357.0 -> 0.318, vertex error 6.73 -> 5.95 mm.  The new config's fit runs on the composed closures and takes 16 s
    or more (a minute was seen): the capture is the one the sweep rule is stated on, so it is not shrunk."""
    from uuo_mocap_amd.metrics import compute_rotation_accel_error

    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50)
    gt_rot = torch.from_numpy(np.asarray(seq.gt["rot"]))[:, 1:].double()
    gt_verts = torch.from_numpy(seq.gt["verts"])
    res = {}
    for name in ("video_mocap", "video_mocap_rotsmooth"):
        out = _fit(seq, name, smpl, dev)
        r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                        out["trans"].cpu().float())
        rot = out["pose_body"].cpu().double()
        res[name] = {"leaf": float(compute_rotation_accel_error(rot, gt_rot, 30.0, LEAF_JOINT_ROWS)),
                     "all": float(compute_rotation_accel_error(rot, gt_rot, 30.0)),
                     "vertex_m": float((r["vertices"] - gt_verts).norm(dim=-1).mean())}
        for k, v in res[name].items():
            record_property("%s_%s" % (name, k), v)
    a, b = res["video_mocap"], res["video_mocap_rotsmooth"]
    print("OBS pose accel (default capture): rotation-acceleration error leaf %.3f -> %.3f, all %.3f -> %.3f; vertex error "
          "%.2f -> %.2f mm" % (a["leaf"], b["leaf"], a["all"], b["all"], 1e3 * a["vertex_m"], 1e3 * b["vertex_m"]))
    assert b["vertex_m"] <= a["vertex_m"] + 5e-4, res
    assert b["leaf"] < a["leaf"], res
