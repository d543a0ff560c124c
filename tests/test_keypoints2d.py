"""EXTENSION: the 2D key-point reprojection term (stages.{chamfer,marker}.losses.keypoints_2d) on the host:
the float64 restatement (tests/keypoints2d_ref64.py) against the closed form and difference quotients, the package's torch term
against the restatement, exact zeros of invalid pairs, config and record parsing, routing, and the 2D-prior hypothesis as a
record (reprojection.world_keypoints_2d)."""
import copy

import numpy as np
import pytest
import torch

from keypoints2d_ref64 import closed_form64, evidence, keypoints2d64, keypoints2d_grad64, make_camera, project64
from uuo_mocap_amd.config import packaged_config

INF = float("inf")


def _joints(F, seed):
    """z-up joint clouds [F, 24, 3] float64 of a person's size, a metre above the origin"""
    gen = torch.Generator().manual_seed(seed)
    J = 0.35 * torch.randn(F, 24, 3, generator=gen, dtype=torch.float64)
    J[..., 2] += 1.0
    return J


def _cfg(name="video_mocap", **stages):
    cfg = packaged_config(name)
    for stage, keys in stages.items():
        for k, v in keys.items():
            if k == "keypoints_2d_block":
                cfg["stages"][stage]["keypoints_2d"] = v
            else:
                cfg["stages"][stage]["losses"][k] = v
    return cfg


def _record(F, seed=3):
    return {k: v.float() for k, v in evidence(_joints(F, seed).numpy(), seed).items()}


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("sigma", [0.0, 8.0])
def test_restatement_autograd_matches_the_closed_form_and_difference_quotients(sigma):
    """tests/test_pose_accel.py's bounds for its own restatement: autograd against the closed form to 1e-13 of the largest
    entry, central difference quotients (h = 1e-6) to 1e-7 + 1e-6 |quotient|."""
    F = 5
    J = _joints(F, 11)
    rec = evidence(J.numpy(), 11)
    cam, y, c = rec["camera"], rec["targets"], rec["confidence"]
    loss, g = keypoints2d_grad64(J, cam, y, c, 3.0, sigma, 0.1)
    closed_loss, closed = closed_form64(J, cam, y, c, 3.0, sigma, 0.1)
    assert loss == pytest.approx(closed_loss, rel=1e-13)
    assert float(np.abs(g.numpy() - closed).max()) <= 1e-13 * max(1.0, float(np.abs(closed).max()))
    assert float(np.abs(closed).max()) > 1e-4
    zero = (c == 0).numpy()
    assert zero.any() and not closed[zero].any() and not g.numpy()[zero].any()
    h = 1e-6
    for f, j, k in [(0, 1, 0), (1, 5, 1), (2, 9, 2), (3, 17, 0), (4, 22, 2), (4, 3, 1)]:
        assert float(c[f, j]) > 0
        Jp, Jm = J.clone(), J.clone()
        Jp[f, j, k] += h
        Jm[f, j, k] -= h
        fd = (float(keypoints2d64(Jp, cam, y, c, 3.0, sigma, 0.1)) - float(keypoints2d64(Jm, cam, y, c, 3.0, sigma, 0.1))) / (2 * h)
        assert abs(fd - float(g[f, j, k])) <= 1e-7 + 1e-6 * abs(fd), (f, j, k, fd, float(g[f, j, k]))


# ------------------------------------------------------------------------------------------------ 2. the package's term
@pytest.mark.parametrize("sigma", [0.0, 8.0])
@pytest.mark.parametrize("weights", [False, True])
def test_package_term_matches_the_restatement(sigma, weights):
    """losses.keypoints_2d_loss in float64 against the restatement to rel 1e-12, loss and gradient; with a joint-weight table the
    confidences are multiplied first (terms.armed_keypoints), as the solvers do."""
    from uuo_mocap_amd.losses import keypoints_2d_loss
    from uuo_mocap_amd.terms import armed_keypoints

    F = 6
    J = _joints(F, 12)
    rec = evidence(J.numpy(), 12)
    cam, y, c = rec["camera"], rec["targets"], rec["confidence"]
    if weights:
        jw = [0.0 if j == 4 else 0.5 + 0.1 * j for j in range(24)]
        kp = {"w": 2.5, "sigma": sigma, "min_depth": 0.1, "joint_weights": jw}
        armed = armed_keypoints({k: v.float() for k, v in rec.items()}, kp)
        assert torch.equal(armed["confidence"], (rec["confidence"].float() * torch.tensor(jw)[None]))
        c = c * torch.tensor(jw, dtype=torch.float64)[None]
    ref_loss, ref_g = keypoints2d_grad64(J, cam, y, c, 2.5, sigma, 0.1)
    leaf = J.clone().requires_grad_(True)
    loss = keypoints_2d_loss(leaf, cam, y, c, 2.5, sigma, 0.1)
    (g,) = torch.autograd.grad(loss, [leaf])
    assert float(loss.detach()) == pytest.approx(ref_loss, rel=1e-12)
    assert float((g - ref_g).abs().max()) <= 1e-12 * float(ref_g.abs().max())
    extra = torch.cat([leaf.detach(), torch.full((F, 21, 3), 7.0, dtype=torch.float64)], dim=1)  # joints 24 .. 44 are not read
    assert float(keypoints_2d_loss(extra, cam, y, c, 2.5, sigma, 0.1)) == float(loss.detach())


# ------------------------------------------------------------------------------------------------ 3. invalid pairs
def test_invalid_pairs_give_exact_zeros():
    """confidence 0, p_z one ulp below min_depth and p_z < 0 give an exact 0 loss and zero gradient rows, in the package's term
    and in the restatement; every other joint lies at p_z >= 1."""
    from uuo_mocap_amd.losses import keypoints_2d_loss

    F, min_depth = 2, 0.25
    J = _joints(F, 13)
    J[..., 1] += 4.0
    # a camera whose depth is world y itself, bit for bit: A's third row is (0, 1, 0) and b_z = 0, so p_z = 0 x + 1 y + 0 z + 0
    cam = make_camera(J.numpy(), swing=0.0)
    cam[:, 11] = 0.0
    below = float(np.nextafter(min_depth, -INF))
    J[0, 3, 1] = below
    J[0, 8, 1] = min_depth       # (exactly at min_depth: valid)
    J[1, 5, 1] = -2.0
    p, _ = project64(J, cam)
    assert float(p[0, 3, 2]) == below and float(p[0, 8, 2]) == min_depth and float(p[1, 5, 2]) == -2.0
    rec = evidence(J.numpy(), 13, zero_every=0)
    y, c = rec["targets"], rec["confidence"].clone()
    c[1, 11] = 0.0
    invalid = torch.zeros(F, 24, dtype=torch.bool)
    invalid[0, 3] = float(p[0, 3, 2]) < min_depth
    invalid[1, 5] = invalid[1, 11] = True
    assert int(invalid.sum()) == 3, "the depth one ulp below min_depth did not survive the placement"
    others = p[..., 2][~invalid]
    assert float(others.min()) >= min_depth and float(p[..., 2][~invalid & (torch.arange(24)[None] != 8)].min()) >= 1.0
    y = torch.where(invalid[..., None], torch.zeros_like(y), y)   # (a target a long way off: it must not matter)
    for sigma in (0.0, 8.0):
        leaf = J.clone().requires_grad_(True)
        loss = keypoints_2d_loss(leaf, cam, y, c, 1.0, sigma, min_depth)
        (g,) = torch.autograd.grad(loss, [leaf])
        assert torch.isfinite(g).all() and not g[invalid].any() and g[~invalid].abs().sum(-1).min() > 0
        ref_loss, ref_g = keypoints2d_grad64(J, cam, y, c, 1.0, sigma, min_depth)
        assert float(loss.detach()) == pytest.approx(ref_loss, rel=1e-12) and not ref_g[invalid].any()
        only = torch.where(invalid, c, torch.zeros_like(c))       # nothing but the invalid pairs: an exact 0
        leaf = J.clone().requires_grad_(True)
        loss = keypoints_2d_loss(leaf, cam, y, only, 1.0, sigma, min_depth)
        (g,) = torch.autograd.grad(loss, [leaf])
        assert float(loss.detach()) == 0.0 and not g.any()


# ------------------------------------------------------------------------------------------------ 4. parser and record
def test_parser_accepts_and_refuses():
    from uuo_mocap_amd.terms import stage_keypoints_2d

    for stage in ("chamfer", "marker"):
        assert stage_keypoints_2d(_cfg(), stage) == {"w": 0.0, "sigma": 0.0, "min_depth": 0.1, "joint_weights": None}
        assert stage_keypoints_2d(_cfg(**{stage: {"keypoints_2d": None}}), stage)["w"] == 0.0
        got = stage_keypoints_2d(_cfg(**{stage: {"keypoints_2d": 3, "keypoints_2d_block": {"sigma": 8, "joint_weights": [1] * 24}}}), stage)
        assert got == {"w": 3.0, "sigma": 8.0, "min_depth": 0.1, "joint_weights": [1.0] * 24}
        assert stage_keypoints_2d(_cfg(**{stage: {"keypoints_2d": 1.0, "keypoints_2d_block": {}}}), stage)["min_depth"] == 0.1
        for bad in (-1.0, -1e-30, INF, -INF, float("nan")):
            with pytest.raises(ValueError, match="keypoints_2d"):
                stage_keypoints_2d(_cfg(**{stage: {"keypoints_2d": bad}}), stage)
        bad_blocks = [[], "x", {"sigma": 0.0, "depth": 1.0}, {"sigma": -1.0}, {"sigma": INF}, {"sigma": "8"}, {"sigma": True},
                      {"sigma": 1e-30}, {"min_depth": 0.0}, {"min_depth": -0.1}, {"min_depth": INF}, {"min_depth": None},
                      {"joint_weights": [1.0] * 23}, {"joint_weights": [1.0] * 23 + [-1.0]}, {"joint_weights": [1.0] * 23 + [INF]},
                      {"joint_weights": 1.0}, {"joint_weights": [1.0] * 23 + ["1"]}]
        for blk in bad_blocks:
            with pytest.raises(ValueError, match="keypoints_2d"):
                stage_keypoints_2d(_cfg(**{stage: {"keypoints_2d": 1.0, "keypoints_2d_block": blk}}), stage)


def test_record_check_accepts_and_refuses():
    from uuo_mocap_amd.terms import armed_keypoints, check_keypoints_2d

    F = 4
    rec = _record(F)
    assert check_keypoints_2d(None) is None and check_keypoints_2d(None, 7) is None
    out = check_keypoints_2d({k: v.double().numpy() for k, v in rec.items()}, F)
    assert all(out[k].dtype == torch.float32 and torch.equal(out[k], rec[k]) for k in rec)

    def edit(key, fn):
        r = {k: v.clone() for k, v in rec.items()}
        r[key] = fn(r[key])
        return r

    def setv(idx, v):
        def fn(t):
            t[idx] = v
            return t
        return fn

    bad = [edit("camera", lambda t: t[:, :15]), edit("camera", lambda t: t[:3]), edit("targets", lambda t: t[:, :23]),
           edit("targets", lambda t: t[..., :1]), edit("confidence", lambda t: t[:, :23]), edit("confidence", lambda t: t[:3]),
           edit("confidence", lambda t: t[..., None]), edit("camera", setv((1, 12), INF)), edit("targets", setv((0, 0, 1), float("nan"))),
           edit("confidence", setv((2, 3), float("nan"))), edit("confidence", setv((2, 3), -0.5)),
           {k: rec[k] for k in ("camera", "targets")}, dict(rec, extra=rec["camera"]), [rec["camera"]], "record"]
    for r in bad:
        with pytest.raises(ValueError, match="keypoints_2d"):
            check_keypoints_2d(r, F)
    with pytest.raises(ValueError, match="keypoints_2d"):
        check_keypoints_2d(rec, F + 1)
    # what is left of a record: nothing without one, at weight 0, or when no confidence * joint weight is positive
    kp = {"w": 1.0, "sigma": 0.0, "min_depth": 0.1, "joint_weights": None}
    assert armed_keypoints(None, kp) is None and armed_keypoints(rec, dict(kp, w=0.0)) is None
    assert armed_keypoints(dict(rec, confidence=torch.zeros(F, 24)), kp) is None
    only5 = dict(rec, confidence=torch.zeros(F, 24))
    only5["confidence"][:, 5] = 1.0
    assert armed_keypoints(only5, dict(kp, joint_weights=[1.0] * 5 + [0.0] + [1.0] * 18)) is None
    assert armed_keypoints(only5, kp)["confidence"] is only5["confidence"]


# ------------------------------------------------------------------------------------------------ 5. the part stage
def test_stage_problems_validate_and_the_part_stage_refuses_the_key():
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem

    with pytest.raises(ValueError, match="keypoints_2d"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"keypoints_2d": -2.0}))
    with pytest.raises(ValueError, match="keypoints_2d"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"keypoints_2d": 1.0, "keypoints_2d_block": {"sigma": -1.0}}))
    with pytest.raises(ValueError, match="keypoints_2d"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"keypoints_2d": 1.0}), keypoints_2d={"camera": torch.zeros(2, 16)})
    with pytest.raises(NotImplementedError, match="soft-assignment closure"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"keypoints_2d": 1.0, "soft_chamfer": 10.0}), keypoints_2d=_record(3))
    with pytest.raises(NotImplementedError, match="keypoints_2d"):
        PartProblem(None, None, None, None, None, None, _cfg(part={"keypoints_2d": 1.0}))


# ------------------------------------------------------------------------------------------------ 6. routes
def test_routes_on_the_host():
    from uuo_mocap_amd.optimization import lockstep_supported
    from uuo_mocap_amd.terms import KEYPOINTS, TERMS, StageTerms, stage_route

    assert TERMS.index(KEYPOINTS) == len(TERMS) - 2 and TERMS[-1].name == "the pose-acceleration term"
    F = 5
    rec = _record(F)
    for stage in ("chamfer", "marker"):
        plain, on = _cfg(), _cfg(**{stage: {"keypoints_2d": 2.0}})
        route = lambda t, **k: stage_route(t, on_device=True, sharded=False, placement="one_hot" if stage == "marker" else None, **k)
        # key on without a record: the plain route, nothing armed
        t = StageTerms(on, stage)
        assert t.on(KEYPOINTS) and t.arm_keypoints(None, F) is None and not t.active(KEYPOINTS) and t.fused(KEYPOINTS)
        assert route(t) == route(StageTerms(plain, stage)) == "fused"
        off = StageTerms(dict(on, execution={"keypoints_fused": False}), stage)
        assert route(off) == "fused"                                    # nothing to compose without a record
        # weight 0 or all-zero confidences: nothing armed either
        assert StageTerms(_cfg(**{stage: {"keypoints_2d": 0.0}}), stage).arm_keypoints(rec, F) is None
        assert StageTerms(on, stage).arm_keypoints(dict(rec, confidence=torch.zeros(F, 24)), F) is None
        # with a record: fused on the device facts, composed with the switch off
        t = StageTerms(on, stage)
        assert t.arm_keypoints(rec, F) is not None and t.active(KEYPOINTS)
        assert route(t) == "fused"
        off.arm_keypoints(rec, F)
        assert not off.fused(KEYPOINTS) and route(off) == "composed"
        tail = off.composed_tail(on["stages"][stage]["losses"], None, None)
        assert [kind for kind, _ in tail] == ["joints"]
        J = _joints(F, 21)
        want = keypoints2d64(J, *(rec[k].double() for k in ("camera", "targets", "confidence")), 2.0, 0.0, 0.1)
        assert float(tail[0][1](J)) == pytest.approx(float(want), rel=1e-12)
        # sharding refuses, lock-step batches do not carry the term
        assert stage_route(t, on_device=True, sharded=True, placement="one_hot" if stage == "marker" else None) == "sharded"
        with pytest.raises(NotImplementedError, match="keypoints_2d.*frame-block sharding"):
            t.refuse_sharded()                                          # (what the sharded solve does first)
        StageTerms(on, stage).refuse_sharded()                          # the key without a record: no refusal, as without the key
        assert lockstep_supported(plain, stage) and not lockstep_supported(on, stage)
        assert lockstep_supported(_cfg(**{stage: {"keypoints_2d": 0.0}}), stage)
    # soft_chamfer + an armed record: the fused soft closure cannot carry it, the call goes composed (no refusal)
    soft = _cfg(chamfer={"keypoints_2d": 2.0, "soft_chamfer": 10.0})
    t = StageTerms(soft, "chamfer")
    assert stage_route(t, on_device=True, sharded=False) == "fused"     # (the fused soft closure, without a record)
    t.arm_keypoints(rec, F)
    assert stage_route(t, on_device=True, sharded=False) == "composed"


def test_optim_entry_points_hand_the_record_on(monkeypatch):
    """optim_chamfer / optim_markers with a record reach the fused problem with the armed record on their StageTerms"""
    from uuo_mocap_amd import optimization as opt

    F, M, V = 5, 4, 6890
    rec = _record(F)
    seen = {}

    class Reached(Exception):
        pass

    def terminal(name):
        def fn(*a, **k):
            seen[name] = k["stage_terms"].keypoints
            raise Reached(name)
        return fn

    for name in ("ChamferProblem", "MarkerProblem", "_optim_chamfer_general", "_optim_markers_general"):
        monkeypatch.setattr(opt, name, terminal(name))

    class _Smpl:
        class device_model:
            V = 6890

    z = torch.zeros
    head = (z(F, M, 3), z(F, 23, 3, 3), z(F, 23, 3, 3), z(1, 10), z(1, 10), z(F, 1, 3, 3), z(F, 3))
    one_hot = z(M, V)
    one_hot[:, 0] = 1.0
    on = _cfg(chamfer={"keypoints_2d": 2.0}, marker={"keypoints_2d": 2.0})
    with pytest.raises(Reached, match="ChamferProblem"):
        opt.optim_chamfer(*head, z(F), z(F, M, dtype=torch.long), None, on, keypoints_2d=rec)
    with pytest.raises(Reached, match="MarkerProblem"):
        opt.optim_markers(*head, one_hot, z(F), _Smpl, on, keypoints_2d=rec)
    assert all(torch.equal(seen[n]["confidence"], rec["confidence"]) for n in ("ChamferProblem", "MarkerProblem"))
    off = dict(on, execution={"keypoints_fused": False})
    with pytest.raises(Reached, match="_optim_chamfer_general"):
        opt.optim_chamfer(*head, z(F), z(F, M, dtype=torch.long), None, off, keypoints_2d=rec)
    with pytest.raises(Reached, match="_optim_markers_general"):
        opt.optim_markers(*head, one_hot, z(F), _Smpl, off, keypoints_2d=rec)
    with pytest.raises(Reached, match="ChamferProblem"):
        opt.optim_chamfer(*head, z(F), z(F, M, dtype=torch.long), None, off)          # no record: the plain route
    assert seen["ChamferProblem"] is None
    with pytest.raises(ValueError, match="keypoints_2d"):
        opt.optim_chamfer(*head, z(F), z(F, M, dtype=torch.long), None, on, keypoints_2d=_record(F + 1))


# ------------------------------------------------------------------------------------------------ 7. the 2D-prior hypothesis
def test_world_keypoints_2d_is_the_part_stages_projection(tables):
    """On SmplInferenceRef in float64: perspective_projection of the record's A J_w + b equals markers_utils.part_extra_losses'
    kp[:, :24] expression (z_angle = 0), restated with the same betas, to 1e-12."""
    from oracle.smpl_ref import SmplInferenceRef
    from uuo_mocap_amd.reprojection import convert_mocap_pos_to_hmr_pos, perspective_projection, world_keypoints_2d
    from uuo_mocap_amd.synthetic import make_sequence

    F = 6
    smpl64 = SmplInferenceRef(tables).double()
    seq = make_sequence(tables, seed=4, num_frames=F, num_markers=8)
    pose, root = seq.img_smpl.pose_body.double(), seq.img_smpl.root_orient.double()
    betas = seq.img_smpl.betas.double().mean(dim=0, keepdim=True)
    trans = torch.from_numpy(seq.gt["trans"]).double()
    gen = torch.Generator().manual_seed(9)
    camera = {"joints_2d_gt": torch.rand(F, 45, 2, generator=gen, dtype=torch.float64),
              "focal_length": torch.tensor([[7.8, 8.1]], dtype=torch.float64),
              "camera_center": 0.05 * torch.randn(F, 2, generator=gen, dtype=torch.float64),
              "cam_trans": torch.tensor([[0.3, -6.0, 1.1]], dtype=torch.float64),
              "reproject_mask": torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 0.0], dtype=torch.float64)}
    eye = torch.eye(3, dtype=torch.float64)
    with torch.no_grad():
        j0 = smpl64(eye.expand(1, 23, 3, 3), betas, eye.expand(1, 1, 3, 3), torch.zeros(1, 3, dtype=torch.float64))["joints"][0, 0]
        rec = world_keypoints_2d(camera, j0)
        # the part stage's expression (part_extra_losses, z_angle = 0: the yaw about the camera is the identity)
        correction = torch.tensor([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]], dtype=torch.float64).expand(F, 1, 3, 3)
        hmr_cam_trans = convert_mocap_pos_to_hmr_pos(camera["cam_trans"]).expand(F, 3)
        joints = smpl64(pose, betas.expand(F, 10), torch.linalg.inv(correction) @ root, convert_mocap_pos_to_hmr_pos(trans))["joints"]
        kp = perspective_projection(joints, hmr_cam_trans, camera["focal_length"].expand(F, 2), camera["camera_center"],
                                    eye.expand(F, 3, 3)) + 0.5
        # the record on the world joints
        Jw = smpl64(pose, betas.expand(F, 10), root, trans)["joints"][:, :24]
        cam = rec["camera"]
        p = torch.einsum("fab,fjb->fja", cam[:, :9].reshape(F, 3, 3), Jw) + cam[:, None, 9:12]
        u = perspective_projection(p, torch.zeros(F, 3, dtype=torch.float64), cam[:, 12:14], cam[:, 14:16])
    assert float((u - kp[:, :24]).abs().max()) <= 1e-12
    _, u64 = project64(Jw, cam)
    assert float((u64 - kp[:, :24]).abs().max()) <= 1e-12
    per_frame = world_keypoints_2d(dict(camera, cam_trans=camera["cam_trans"].expand(F, 3).contiguous()), j0)   # (as the stage returns it)
    assert all(torch.equal(per_frame[k], rec[k]) for k in rec)
    assert torch.equal(rec["targets"], camera["joints_2d_gt"][:, :24])
    assert torch.equal(rec["confidence"], camera["reproject_mask"][:, None].expand(F, 24))
    from uuo_mocap_amd.terms import check_keypoints_2d

    assert check_keypoints_2d(rec, F)["camera"].shape == (F, 16)


def test_synthetic_keypoints_and_the_elbow_capture(tables):
    from uuo_mocap_amd.synthetic import ELBOW_WINDOW, make_sequence, synthetic_camera, synthetic_keypoints_2d
    from uuo_mocap_amd.terms import check_keypoints_2d

    F = 60
    plain = make_sequence(tables, seed=0, num_frames=F, num_markers=20)
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=20, elbow_error=True)
    w0, w1 = seq.gt["elbow_window"]
    assert (w0, w1) == (6, 6 + ELBOW_WINDOW)
    diff = (seq.img_smpl.pose_body - plain.img_smpl.pose_body).abs().amax(dim=(2, 3))          # [F, 23]
    assert not diff[:w0].any() and not diff[w1:].any() and not diff[:, [j for j in range(23) if j != 17]].any()
    assert diff[w0:w1, 17].min() > 0.05
    for k in ("verts", "joints", "trans"):
        assert np.array_equal(seq.gt[k], plain.gt[k])
    pts, pts0 = np.asarray(seq.markers.get_points()), np.asarray(plain.markers.get_points())
    assert np.array_equal(pts[:w0], pts0[:w0]) and np.array_equal(pts[w1:], pts0[w1:]) and (pts[w0:w1] != pts0[w0:w1]).any()
    with pytest.raises(ValueError, match="elbow_error"):
        make_sequence(tables, seed=0, num_frames=20, num_markers=20, elbow_error=True)
    exact = check_keypoints_2d(synthetic_keypoints_2d(seq, noise=0.0), F)
    noisy = check_keypoints_2d(synthetic_keypoints_2d(seq, noise=2.0, seed=1, dropped_frames=[3, 4]), F)
    cam = torch.from_numpy(synthetic_camera(seq))
    assert torch.allclose(exact["camera"].double(), cam[None].expand(F, 16), rtol=1e-6)
    p, u = project64(torch.from_numpy(seq.gt["joints"][:, :24]).double(), exact["camera"].double())
    assert float(p[..., 2].min()) > 2.0 and float((u - exact["targets"].double()).abs().max()) < 1e-3
    d = (noisy["targets"] - exact["targets"]).double()
    assert 1.5 < float(d.std()) < 2.5 and abs(float(d.mean())) < 0.2
    assert not noisy["confidence"][[3, 4]].any() and bool((noisy["confidence"][[0, 1, 2, 5]] == 1).all())
