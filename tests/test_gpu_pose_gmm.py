"""EXTENSION: the mixture pose prior on the body pose (stages.{chamfer,marker}.losses.pose_gmm, uuo_fit_set_pose_gmm, k_pose_gmm) on
the MI355X -- the fused closures against float64 (stage_ref64's restatement of the closure plus the loop-written float64 term
of tests/pose_gmm_ref64.py), the term alone beside the composed fp32 term's own error, the winners, the buffer it shares with
the joint-angle limits, the pose acceleration and the weighted prior, hand-built poses, the invariances (off is off, two
evaluations, four in flight, a frame alone and inside a longer sequence, a second mixture and back), fused against composed
solves, the refusals, and a fit with video_mocap_gmm.yaml."""
import copy
import itertools
import math
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import stages_ref  # noqa: E402
from pose_gmm_ref64 import energies_np, find_case, gs64, make_mixture, raw_from_theta, rodrigues, term_np  # noqa: E402
from capsules_ref64 import _caps_grad, _lists as _cap_lists  # noqa: E402
from floor_ref64 import _contacts, _plane, _vids  # noqa: E402
from gpu_support import (R_CHAMFER, R_MARKER, U_TABLE, W_CAPS_C, W_CAPS_M, W_KP_C, W_KP_M, W_LIM_C, W_LIM_M,  # noqa: E402,F401
                         W_PACC_C, W_PACC_M, _inputs, _marker_x, _rel_err, _three_corners, dev, smpl, smpl64)
from joint_limits_ref64 import _cfg as _lim_cfg, _lim_grad, _tables as _lim_tables  # noqa: E402
from keypoints2d_ref64 import _kp_grad, _record, _with_key  # noqa: E402
from pose_accel_ref64 import pose_accel_grad64  # noqa: E402
from prior_confidence_ref64 import _prior64, _weight_tables, _without  # noqa: E402
from stage_ref64 import (_chamfer_forward64, _float64, _heights64, _marker_forward64, ref_chamfer64 as _ref_chamfer,  # noqa: E402
                         ref_marker64 as _ref_marker)
from uuo_mocap_amd.body_model import pose_log_vector, prepare_pose_mixture  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

FPB = 8   # UUO_GMM_FPB: the frames a block of k_pose_gmm takes
# weights of the parity checks.  d E / d theta = A (A^T d) has entries of 1 / sigma size, 2 .. 50 per component on the two
# recipes; times w / F it has to stand beside the data term's ~ 0.03 / F in pose space (tests/test_gpu_joint_limits.py): 0.01 on
# the chamfer closure and 0.001 on the marker closures, whose data term is ten times smaller, keep the term's share of the
# gradient far above the 2e-2 the check asks for while the data term and the priors still show in the compared digits.
W_CHAMFER, W_MARKER = 0.01, 0.001
# ... and beside every other setting at once -- the capsules at test_gpu_capsules' 100 / 10, the floor and foot-lock terms, the key
# points -- whose gradients are ten and more times the plain closure's: ten times the weight, for the same share
W_ALL_C, W_ALL_M = 0.1, 0.01


def _set_gmm(cfg, w_chamfer, w_marker):
    cfg = copy.deepcopy(cfg)
    for stage, w in (("chamfer", w_chamfer), ("marker", w_marker)):
        if w is not None:
            cfg["stages"][stage]["losses"]["pose_gmm"] = w
        cfg["stages"][stage].setdefault("floor_height", 0.0)   # (the stage reference reads it)
    return cfg


def _alone(cfg):
    cfg["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_pose_body=0.0, reg_betas=0.0)
    cfg["stages"]["marker"]["losses"].update(marker=0.0, reg_pose_body=0.0, reg_betas=0.0)
    return cfg


class _Planted:
    """One (kind, K, F): a mixture and raw float32 body poses planted on its components (pose_gmm_ref64.find_case: the first
    seed that meets the float64 preconditions), which are asserted again on what the closures see -- the float32 raw entries
    through the float64 Gram-Schmidt map and the float32 mixture arrays -- before anything is compared."""

    def __init__(self, kind, K, F, seed0=0):
        self.mix, theta, self.seed = find_case(kind, K, F, seed0)
        self.raw = torch.from_numpy(raw_from_theta(theta, np.random.default_rng(self.seed + 77))).float()
        self.means, self.chol, self.offsets = (a.astype(np.float64) for a in prepare_pose_mixture(**self.mix))
        th = pose_log_vector(gs64(self.raw.double().numpy()))
        ang = np.linalg.norm(th.reshape(F, 23, 3), axis=-1)
        assert ang.min() >= 1e-2 and ang.max() <= 2.9, "a joint's angle outside [1e-2, 2.9]: pick another seed"
        self.energies = energies_np(th, self.means, self.chol, self.offsets)
        self.winners = self.energies.argmin(axis=1)
        assert len(set(self.winners.tolist())) == min(F, K), "the winners are not min(F, K) distinct components"
        if K > 1:
            srt = np.sort(self.energies, axis=1)
            self.gap = float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min())
            assert self.gap >= 1e-2, "a second-best energy within 1e-2 relative of the best: pick another seed"

    def term64(self, raw, w, n, pose_slice):
        """float64 loss, flat gradient [n] in the closure's packing and winners: the loop-written term on the float64
        Gram-Schmidt of raw [F, 23, 3, 3], its d loss / d R taken through the map by autograd"""
        with _float64():
            leaf = raw.detach().cpu().double().clone().requires_grad_(True)
            R = stages_ref.normalize_rot(leaf)
            loss, gR, _, win, _ = term_np(R.detach().numpy(), self.means, self.chol, self.offsets, w)
            (g,) = torch.autograd.grad((R * torch.from_numpy(gR)).sum(), [leaf])
        out = np.zeros(n)
        out[pose_slice] = g.reshape(-1).numpy()
        return loss, out, win


def _winners(prob):
    """the winning component per frame of the last evaluation on the problem's workspace (debug hook)"""
    from uuo_mocap_amd import _lib

    out = np.zeros(prob.F, dtype=np.int32)
    assert _lib.load_debug().uuo_debug_pose_gmm_state(prob.fit, out.ctypes.data, None) == 0
    return out


def _shares(prob):
    """the [F] loss shares behind lim_g's gradients after the last evaluation on the problem's workspace (debug hook): the
    mixture's w E / F alone when no other term of that buffer is on"""
    from uuo_mocap_amd import _lib

    out = np.zeros(prob.F, dtype=np.float32)
    assert _lib.load_debug().uuo_debug_pose_gmm_state(prob.fit, None, out.ctypes.data) == 0
    return out


def _composed32(case, raw, w):
    """the composed closures' term (losses.pose_gmm_loss on normalize_rot of the raw entries) through float32 autograd"""
    from uuo_mocap_amd.losses import pose_gmm_loss
    from uuo_mocap_amd.transforms import normalize_rot

    leaf = raw.detach().float().clone().requires_grad_(True)
    loss = pose_gmm_loss(normalize_rot(leaf), case.means, case.chol, case.offsets, w)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss), g.double().reshape(-1).numpy()


def _closures(smpl, tables, dev, F, M, seed, pose):
    """the three closure kinds of a case on the body pose `pose`: name -> (make(cfg, **kw), x(problem), pose slice, float64
    rest(cfg, x, nn))"""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, _, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts, svids = _contacts(F, seed), _vids(tables, 6)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (markers.to(dev), o_pose.to(dev), o_betas.to(dev))
    sl_c, sl_m = slice(4 * F + 10, 211 * F + 10), slice(0, 207 * F)
    out = {"chamfer": (lambda cfg, **kw: ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts, **kw),
                       lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pose.to(dev)), sl_c,
                       lambda cfg, x, nn: _ref_chamfer(stages_smpl64[0], cfg, markers, o_pose, o_betas, root, x, nn, contacts, svids, 3))}
    for name, assign, bary in (("one-hot", mvids, None), ("three-corner", i3, b3)):
        out[name] = (lambda cfg, a=assign, b=bary, **kw: MarkerProblem(smpl, *args, a.to(dev), cfg, bary=None if b is None else b.to(dev),
                                                                        foot_contacts=contacts, **kw),
                     lambda p: _marker_x(p, pose, bp, rp, tp, dev, F, num_markers=M), sl_m,
                     lambda cfg, x, nn, a=assign, b=bary: _ref_marker(stages_smpl64[0], tables, cfg, markers, o_pose, o_betas, x, a, b,
                                                                      contacts, svids, 3, M))
    return out, (o_pose, root, contacts)


stages_smpl64 = [None]   # (the module's float64 model, set by the fixture below: the closures' restatements need it)


@pytest.fixture(autouse=True)
def _model64(smpl64):
    stages_smpl64[0] = smpl64


def _parity(smpl, tables, dev, F, K, M, kinds, alone=False, record=None):
    worst = {}
    for kind in kinds:
        case = _Planted(kind, K, F)
        closures, _ = _closures(smpl, tables, dev, F, M, 600 + 37 * F + M, case.raw)
        base = _set_gmm(packaged_config("video_mocap"), None, None)
        cfg, cfg0 = _set_gmm(base, W_CHAMFER, W_MARKER), _set_gmm(base, 0.0, 0.0)
        if alone:
            cfg, cfg0 = _alone(cfg), _alone(cfg0)
        for name, (make, pack, sl, rest) in closures.items():
            w = W_CHAMFER if name == "chamfer" else W_MARKER
            prob, prob0 = make(cfg, pose_mixture=case.mix), make(cfg0)
            assert prob.pose_gmm_on and prob.gmm_w == w and prob.gmm_means.shape == (K, 69) and not prob0.pose_gmm_on
            x = pack(prob)
            loss, grad, nn = prob.evaluate(x)
            win = _winners(prob)
            _, grad0, nn0 = prob0.evaluate(x)
            if name == "chamfer":
                assert torch.equal(nn, nn0), "the term must not change the assignment"
            l0, g0 = rest(cfg0, x, nn)
            lt, gt, win64 = case.term64(x.detach().cpu()[sl].reshape(F, 23, 3, 3), w, x.numel(), sl)
            g = grad.cpu().numpy()
            lo, g_ref = l0 + lt, g0 + gt
            share = _rel_err(g, grad0.cpu().numpy())
            e_loss, e_grad = abs(loss - lo) / abs(lo), _rel_err(g, g_ref)
            tag = (name, kind, F, K, M, alone)
            msg = "OBS pose gmm parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e" % (tag, e_loss, e_grad, share)
            if alone:   # the composed fp32 term's own distance from float64 on the same inputs
                lc, gc = _composed32(case, x.detach().cpu()[sl].reshape(F, 23, 3, 3), w)
                c_loss, c_grad = abs(lc - lt) / abs(lt), _rel_err(gc, gt[sl])
                msg += "; composed fp32 term: loss rel %.2e, gradient rel %.2e" % (c_loss, c_grad)
                worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0.0,) * 4), (e_loss, e_grad, c_loss, c_grad)))
                assert l0 == 0.0 and not g0.any()
            print(msg)
            assert win.tolist() == win64.tolist() == case.winners.tolist(), tag
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
            assert e_grad < 2e-4, tag
            assert share > 2e-2, tag
    if record is not None:
        for kind, v in worst.items():
            for key, val in zip(("kernel_loss", "kernel_grad", "composed_loss", "composed_grad"), v):
                record("%s_%s" % (kind, key), val)


# ------------------------------------------------------------------------------------------------ 1. closure parity
# a lone frame, a block's idle tail, a full block, a second block with one frame, a third block with one frame
SHAPES = [(F, K, M) for F in (1, FPB - 1, FPB, FPB + 1, 2 * FPB + 1) for K in (1, 2, 8, 16) for M in (10, 50)]


@pytest.mark.parametrize("F,K,M", SHAPES)
def test_gmm_closures_match_float64(smpl, tables, dev, F, K, M):
    """Loss rtol 2e-5, gradient relative error < 2e-4 against float64 (test_gpu_floor's restatement of the closures plus the
    term's own, whose gradients add), the term changes the gradient by more than 2e-2 relative, and the kernel's winners are
    float64's -- chamfer, one-hot and three-corner closures, the far and the close mixture.  The float64 preconditions are
    asserted first (_Planted)."""
    _parity(smpl, tables, dev, F, K, M, ("far", "close"))


@pytest.mark.parametrize("F,K", [(1, 1), (FPB - 1, 2), (FPB + 1, 8), (2 * FPB + 1, 16)])
def test_the_term_alone_matches_float64(smpl, tables, dev, F, K, record_property):
    """w_data = 0 and both priors 0: loss and gradient ARE the term, at the same two bounds; beside them the composed fp32 term's
    own distance from float64 on the same inputs (printed and recorded: DESIGN 4z quotes the maxima)."""
    _parity(smpl, tables, dev, F, K, 10, ("far", "close"), alone=True, record=record_property)


# ------------------------------------------------------------------------------------------------ 2. the shared buffer
def _subset_cfg(limits, gmm, pacc, lim_tab):
    cfg = _lim_cfg(lim_tab if limits else None, W_LIM_C if limits else 0.0, W_LIM_M if limits else 0.0, keys=limits)
    cfg["execution"] = {"pose_accel_fused": True}
    for stage, wg, wp, reg in (("chamfer", W_CHAMFER, W_PACC_C, R_CHAMFER), ("marker", W_MARKER, W_PACC_M, R_MARKER)):
        st = cfg["stages"][stage]
        st["losses"]["reg_pose_body"] = reg
        if gmm:
            st["losses"]["pose_gmm"] = wg
        if pacc:
            st["losses"]["pose_accel"] = wp
            st["pose_accel"] = {"joint_weights": list(U_TABLE)}
    return cfg


def test_the_add_chain_for_every_subset(smpl, tables, dev):
    """joint_limits (+-0.2 rad on every component), the mixture, pose_accel (fused) and the prior weights share one buffer: the
    first kernel of an evaluation to reach it writes, the later ones add (k_limit_fwd -> k_pose_gmm -> k_pose_accel ->
    k_prior_conf).  Every one of the 16 subsets at F = FPB + 1, K = 2, chamfer and one-hot closure, one after another on one
    workspace, against the float64 sums at the parity bounds."""
    F, K, M = FPB + 1, 2, 11
    case = _Planted("close", K, F)
    closures, (o_pose, root, _) = _closures(smpl, tables, dev, F, M, 600 + 37 * F + M, case.raw)
    lim_tab = _lim_tables()["full"]
    wtab = _weight_tables(F, 5)["hash"]
    for name in ("chamfer", "one-hot"):
        make, pack, sl, rest = closures[name]
        i = 0 if name == "chamfer" else 1
        x = pack(make(_subset_cfg(False, False, False, lim_tab)))
        raw = x.detach().cpu()[sl].reshape(F, 23, 3, 3)
        for limits, gmm, pacc, prior in itertools.product((False, True), repeat=4):
            cfg = _subset_cfg(limits, gmm, pacc, lim_tab)
            prob = make(cfg, prior_weights=wtab if prior else None, **({"pose_mixture": case.mix} if gmm else {}))
            assert (prob.joint_limits_on, prob.pose_gmm_on, prob.pose_accel_on, prob.prior_conf_on) == (limits, gmm, pacc, prior)
            loss, grad, nn = prob.evaluate(x)
            plain = _without(_subset_cfg(False, False, False, lim_tab))   # (no limits, no pose prior: added below)
            lo, g_ref = rest(plain, x, nn)
            lp, gp = _prior64(x, sl, o_pose, wtab if prior else None, (R_CHAMFER, R_MARKER)[i], x.numel())
            lo, g_ref = lo + lp, g_ref + gp
            if limits:
                with _float64():
                    leaves = (_chamfer_forward64(stages_smpl64[0], x.detach().cpu().double(), root.double(), F)[0]
                              if name == "chamfer" else _marker_forward64(stages_smpl64[0], x.detach().cpu().double()[:219 * F + 10], F)[0])
                ll, gl = _lim_grad(leaves, 3 if name == "chamfer" else 0, lim_tab, (W_LIM_C, W_LIM_M)[i])
                lo, g_ref = lo + ll, g_ref + gl
            if gmm:
                lt, gt, _ = case.term64(raw, (W_CHAMFER, W_MARKER)[i], x.numel(), sl)
                lo, g_ref = lo + lt, g_ref + gt
            if pacc:
                la, ga = pose_accel_grad64(raw, (W_PACC_C, W_PACC_M)[i], U_TABLE)
                lo = lo + la
                g_ref = g_ref.copy()
                g_ref[sl] += ga.reshape(-1).numpy()
            g = grad.cpu().numpy()
            tag = (name, limits, gmm, pacc, prior)
            print("OBS pose gmm add chain %s: loss rel %.2e, gradient rel %.2e" % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref)))
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, g_ref) < 2e-4, tag


def test_with_every_other_setting_on(smpl, tables, dev):
    """sigma, joint_accel + foot_lock, the floor term, the capsules, the key points and latent_offsets all on beside the term, one
    case (F = FPB + 1, K = 2, M = 10), the three closures, at the parity bounds (the same settings all off are the plain parity
    cases above).  The term runs at ten times the parity weights here (W_ALL_C / W_ALL_M = 0.1 / 0.01): the other terms, the
    capsules at 100 / 10 first, bring the closure's gradient to ten and more times the plain one's, and the check that the term
    matters (its share of the gradient above 2e-2) is kept, not lowered."""
    F, K, M = FPB + 1, 2, 10
    seed = 600 + 37 * F + M
    case = _Planted("close", K, F)
    closures, (o_pose, root, contacts) = _closures(smpl, tables, dev, F, M, seed, case.raw)
    _, _, _, _, _, _, (tp, zp, bp, _, rp) = _inputs(tables, F, seed, num_markers=M)
    svids = _vids(tables, 6)
    planes = (_plane(_heights64(stages_smpl64[0], case.raw, bp, root, tp, svids, z=zp), 3, contacts),
              _plane(_heights64(stages_smpl64[0], case.raw, bp, rp, tp, svids), 3, contacts))
    cap_list = _cap_lists(tables)["builder"]
    rec = {}
    for name, (make, pack, sl, rest) in closures.items():
        offs = name != "chamfer"
        i = 0 if name == "chamfer" else 1
        cfg0 = _lim_cfg(None, sigma=0.05, temporal=True, floor=planes, caps=cap_list, offs=offs, keys=False)
        x = pack(make(cfg0))
        n0 = 219 * F + 10
        forward = (lambda: _chamfer_forward64(stages_smpl64[0], x.detach().cpu().double(), root.double(), F)) if name == "chamfer" \
            else (lambda: _marker_forward64(stages_smpl64[0], x.detach().cpu().double()[:n0], F))
        if i not in rec:
            with _float64():
                rec[i] = _record(forward()[1]["joints"][:, :24].detach().numpy(), seed + i)
        cfg0k = _with_key(cfg0, W_KP_C, W_KP_M, 8.0)
        cfg = _set_gmm(cfg0k, W_ALL_C, W_ALL_M)
        prob = make(cfg, pose_mixture=case.mix, keypoints_2d=rec[i])
        assert prob.pose_gmm_on and prob.keypoints_on and prob.capsules_on and prob.floor_on and prob.joint_accel > 0
        assert name == "chamfer" or prob.has_offsets
        loss, grad, nn = prob.evaluate(x)
        _, grad0, _ = make(cfg0k, keypoints_2d=rec[i]).evaluate(x)
        lo, g_ref = rest(cfg0, x, nn)
        pad = 3 * M if offs else 0
        with _float64():
            leaves, out = forward()
        lk, gk = _kp_grad(leaves, out, rec[i], (W_KP_C, W_KP_M)[i], 8.0, pad=pad)
        lc, gc = _caps_grad(leaves, out, cap_list, (W_CAPS_C, W_CAPS_M)[i], pad=pad)
        lt, gt, _ = case.term64(x.detach().cpu()[sl].reshape(F, 23, 3, 3), (W_ALL_C, W_ALL_M)[i], x.numel(), sl)
        lo, g_ref = lo + lk + lc + lt, g_ref + gk + gc + gt
        g = grad.cpu().numpy()
        share = _rel_err(g, grad0.cpu().numpy())
        print("OBS pose gmm with every setting on (%s): loss rel %.2e, gradient rel %.2e, term's share %.2e"
              % (name, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), share))
        np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
        assert _rel_err(g, g_ref) < 2e-4 and share > 2e-2, name


# ------------------------------------------------------------------------------------------------ 3. hand-built poses
def test_identity_and_half_turn_branches_of_the_kernel(smpl, tables, dev):
    """The term alone.  Every joint at the exact identity with non-zero means: kappa = 1, theta = 0, float64's loss and gradient.
    A joint within 5e-6 rad of a half turn: its nine gradient entries are exact zeros and the loss is that of omega_j = 0."""
    F, K, M = 3, 2, 10
    case = _Planted("close", K, F)
    cfg = _alone(_set_gmm(packaged_config("video_mocap"), 1.0, 1.0))
    # --- the identity
    eye = torch.eye(3).repeat(F, 23, 1, 1)
    closures, _ = _closures(smpl, tables, dev, F, M, 777, eye)
    for name in ("chamfer", "one-hot"):
        make, pack, sl, _ = closures[name]
        prob = make(cfg, pose_mixture=case.mix)
        x = pack(prob)
        loss, grad, _ = prob.evaluate(x)
        lt, gt, win = case.term64(eye, 1.0, x.numel(), sl)
        e0 = energies_np(np.zeros((1, 69)), case.means, case.chol, case.offsets)[0]
        assert lt == pytest.approx(e0.min(), rel=1e-12) and np.abs(gt).max() > 1e-2
        np.testing.assert_allclose(loss, lt, rtol=2e-5)
        assert _rel_err(grad.cpu().numpy(), gt) < 2e-4 and _winners(prob).tolist() == win.tolist()
    # --- the half turn: joint 5 (row 4) of every frame within 5e-6 rad of pi about three different axes
    pose = case.raw.clone()
    for f, axis in enumerate(([1.0, 0.0, 0.0], [0.0, 0.6, 0.8], [0.48, -0.6, 0.64])):
        pose[f, 4] = torch.from_numpy(rodrigues(np.asarray(axis) * (math.pi - 5e-6))).float()
    zero = case.raw.clone()
    zero[:, 4] = torch.eye(3)   # omega_j = 0
    closures, _ = _closures(smpl, tables, dev, F, M, 777, pose)
    closures0, _ = _closures(smpl, tables, dev, F, M, 777, zero)
    for name in ("chamfer", "one-hot"):
        make, pack, sl, _ = closures[name]
        prob = make(cfg, pose_mixture=case.mix)
        x = pack(prob)
        loss, grad, _ = prob.evaluate(x)
        gp = grad.cpu()[sl].reshape(F, 23, 9)
        assert not gp[:, 4].any() and gp[:, 3].abs().sum() > 0 and gp[:, 5].abs().sum() > 0
        l0, g0, _ = prob.evaluate(closures0[name][1](prob))
        assert loss == l0                                            # the loss of omega_j = 0, bit for bit
        rest = [j for j in range(23) if j != 4]
        assert torch.equal(gp[:, rest], g0.cpu()[sl].reshape(F, 23, 9)[:, rest])
        lt, gt, _ = case.term64(pose, 1.0, x.numel(), sl)
        np.testing.assert_allclose(loss, lt, rtol=2e-5)
        assert _rel_err(grad.cpu().numpy(), gt) < 2e-4


# ------------------------------------------------------------------------------------------------ 4. invariances
def test_off_is_off_and_on_is_deterministic(smpl, tables, dev):
    """Key absent == weight 0, bit for bit on loss and gradient, for the three closure kinds, on a fresh thread's workspace and
    on one that has just evaluated with the term on (w = 0 after w > 0); two evaluations with the term on are bitwise equal; a
    second mixture on the same workspace replaces the first, and back gives the first's results again; with reg_pose_body 0 the
    third rows of the pose gradient are exact zeros (the compact packing has no slot for them)."""
    F, K, M = 2 * FPB + 1, 8, 11
    case = _Planted("far", K, F)
    other = make_mixture("close", 3, np.random.default_rng(99))
    closures, _ = _closures(smpl, tables, dev, F, M, 123, case.raw)
    absent = _set_gmm(packaged_config("video_mocap"), None, None)
    on, zero = _set_gmm(absent, W_CHAMFER, W_MARKER), _set_gmm(absent, 0.0, 0.0)
    noreg = copy.deepcopy(on)
    for stage in ("chamfer", "marker"):
        noreg["stages"][stage]["losses"]["reg_pose_body"] = 0.0
    for name, (make, pack, sl, _) in closures.items():
        fresh = {}

        def on_fresh_thread():  # workspaces are per thread: this one has never seen the term
            p = make(absent)
            fresh["r"] = p.evaluate(pack(p), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        pw = make(on, pose_mixture=case.mix)
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name
        lf, gf = fresh["r"]
        assert lw > lf and not torch.equal(gw, gf), name
        p2 = make(on, pose_mixture=other)
        l2, g2, _ = p2.evaluate(x, want_nn=False)
        assert l2 != lw and not torch.equal(g2, gw), name        # another mixture, other results
        lw3, gw3, _ = pw.evaluate(x, want_nn=False)              # and back
        assert lw3 == lw and torch.equal(gw3, gw), name
        for tag, cfg in (("absent", absent), ("weight 0", zero)):
            p = make(cfg)
            assert not p.pose_gmm_on, (name, tag)
            pw.evaluate(x, want_nn=False)                        # the workspace has just run with the term on
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)
        _, g, _ = make(noreg, pose_mixture=case.mix).evaluate(x, want_nn=False)
        gp = g[sl].reshape(F, 23, 3, 3)
        assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any(), name


def test_a_frame_alone_and_inside_a_longer_sequence(smpl, tables, dev):
    """Frame t's gradient rows and its share w E / F (read back from the buffer's [F] tail) are bitwise equal at F = t + 1 and
    inside F = 2 FPB + 1 -- whatever block and slot the frame falls into.  The term alone; the weight is 0.5 F, so that w / F is
    the same float in every run.  The shares are also float64's 0.5 E_t to the parity bound."""
    Fl, K, M = 2 * FPB + 1, 8, 10
    case = _Planted("close", K, Fl)
    cfg_for = lambda F: _alone(_set_gmm(packaged_config("video_mocap"), 0.5 * F, 0.5 * F))

    def run(F, name):
        closures, _ = _closures(smpl, tables, dev, F, M, 321, case.raw[:F])
        make, pack, sl, _ = closures[name]
        prob = make(cfg_for(F), pose_mixture=case.mix)
        loss, grad, _ = prob.evaluate(pack(prob), want_nn=False)
        return loss, grad.cpu()[sl].reshape(F, 207), _winners(prob), _shares(prob)

    for name in ("chamfer", "one-hot"):
        _, g_long, w_long, s_long = run(Fl, name)
        assert w_long.tolist() == case.winners.tolist()
        np.testing.assert_allclose(s_long, 0.5 * case.energies.min(axis=1), rtol=2e-5)
        assert (s_long > 0).all() and len(set(s_long.tolist())) == Fl       # (every frame its own share)
        for t in (0, FPB - 2, FPB - 1, FPB, 2 * FPB - 1):
            loss, g, w, s = run(t + 1, name)
            assert torch.equal(g[t], g_long[t]) and w[t] == w_long[t], (name, t)
            assert torch.equal(g, g_long[:t + 1]), (name, t)
            assert s[t].tobytes() == s_long[t].tobytes(), (name, t, float(s[t]), float(s_long[t]))
            assert s.tobytes() == s_long[:t + 1].tobytes(), (name, t)
        # the loss at F = 1 is frame 0's share alone
        loss1, _, _, s1 = run(1, name)
        assert s1[0] == s_long[0] and loss1 == pytest.approx(float(s1[0]), rel=1e-6)


@pytest.mark.parametrize("stage", ["marker", "chamfer"])
def test_four_in_flight_are_bit_identical_to_one(smpl, tables, dev, stage, record_property):
    """parallel.fit_many over 8 problems at F = 2 FPB + 1, 30 evaluations each at perturbed points: every loss and gradient with
    inflight=4 is bitwise equal to the same work with inflight=1 -- 240 evaluations per stage."""
    from uuo_mocap_amd.parallel import fit_many

    F, K, M, N, E = 2 * FPB + 1, 8, 11, 8, 30
    case = _Planted("close", K, F)
    cfg = _set_gmm(packaged_config("video_mocap"), W_CHAMFER, W_MARKER)
    name = "chamfer" if stage == "chamfer" else "one-hot"
    items = [(i, _closures(smpl, tables, dev, F, M, 400 + i, case.raw)[0][name]) for i in range(N)]

    def work(item):
        i, (make, pack, _, _) = item
        p = make(cfg, pose_mixture=case.mix)
        assert p.pose_gmm_on
        x0 = pack(p)
        gen = torch.Generator().manual_seed(i)
        out = []
        for e in range(E):
            x = (x0 + 0.01 * torch.randn(x0.numel(), generator=gen).to(dev)).contiguous()
            loss, grad, _ = p.evaluate(x, want_nn=False)
            out.append((loss, grad.cpu()))
        return out

    one = fit_many(items, work, inflight=1, device=dev)
    four = fit_many(items, work, inflight=4, device=dev)
    wrong = [(i, e) for i in range(N) for e in range(E)
             if one[i][e][0] != four[i][e][0] or not torch.equal(one[i][e][1], four[i][e][1])]
    record_property("evaluations", N * E)
    record_property("evaluations_that_differ", len(wrong))
    assert not wrong, "%d of %d evaluations differ with four in flight; the first: %s" % (len(wrong), N * E, wrong[:5])


# ------------------------------------------------------------------------------------------------ 5. fused vs composed
@pytest.mark.parametrize("F", [7, 300])
def test_fused_and_composed_gmm_solves_agree(smpl, tables, dev, F):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.pose_gmm_fused: False) with the stand-in mixture: the start agrees to 1e-5, the end to 5e-2, and both decrease."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers
    from uuo_mocap_amd.synthetic import pose_mixture

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
        cfg = _set_gmm(packaged_config("video_mocap"), 0.01, 0.001)
        cfg["execution"] = {"pose_gmm_fused": fused}
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 25
        pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
        optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                      root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                      marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg,
                      pose_mixture=pose_mixture())
        sc = dict(last_stats("chamfer"))
        o_pose_m = pose.detach().clone()
        optim_markers(md, pose_body=pose, o_pose_body=o_pose_m, betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                      trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                      smpl_inference=smpl, config=cfg, pose_mixture=pose_mixture())
        out[fused] = (sc, dict(last_stats("marker")))
    (cf, mf), (cc, mc) = out[True], out[False]
    assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
    print("OBS pose gmm fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (F, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=5e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)
    assert final(cc) < first(cc) and final(mc) < first(mc)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_library_and_routes_refuse_the_term_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103)
    md = markers.to(dev)
    mix = make_mixture("close", 3, np.random.default_rng(4))
    means, chol, offsets = prepare_pose_mixture(**mix)

    def arm(p, w=1.0):  # what no config can produce: the library itself must refuse it
        p.gmm_means, p.gmm_chol, p.gmm_offsets, p.gmm_w = means, chol, offsets, w

    # the part stage refuses at evaluation
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    arm(pp)
    with pytest.raises(RuntimeError, match="pose mixture term.*part stage"):
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
    with pytest.raises(RuntimeError, match="pose mixture term.*soft-assignment"):
        ps.evaluate(xs)
    arm(ps, 0.0)
    assert ps.evaluate(xs)[0] == ls0
    # the setter: every bad argument with its own text; off with null pointers
    lib, fit = smpl.device_model.lib, pp.fit

    def call(w=1.0, K=3, a=means, b=chol, c=offsets):
        a, b, c = (None if t is None else np.ascontiguousarray(t, dtype=np.float32) for t in (a, b, c))
        rc = lib.uuo_fit_set_pose_gmm(fit, w, K, *(None if t is None else t.ctypes.data for t in (a, b, c)))
        return rc, (lib.uuo_last_error().decode() if rc else "")

    def edit(t, idx, v):
        u = t.copy()
        u[idx] = v
        return u

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == -22 and text in msg, (kw.keys(), msg)

    assert call() == (0, "")
    for w in (-1.0, float("nan"), float("inf")):
        refused("the weight must be 0 (off) or a positive finite number", w=w)
    for K in (0, -1, 17):
        refused("1 .. 16 components", K=K)
    for k in ("a", "b", "c"):
        refused("a positive weight needs", **{k: None})
    refused("a mean is NaN or not finite", a=edit(means, (1, 5), float("nan")))
    refused("a mean is NaN or not finite", a=edit(means, (1, 5), float("inf")))
    refused("an entry of a factor A_k is NaN or not finite", b=edit(chol, (2, 7, 3), float("nan")))
    refused("an offset is NaN or not finite", c=edit(offsets, 1, float("nan")))
    refused("a diagonal entry of a factor A_k is not positive", b=edit(chol, (2, 7, 7), 0.0))
    refused("a diagonal entry of a factor A_k is not positive", b=edit(chol, (0, 68, 68), -1.0))
    refused("an offset is negative", c=edit(offsets, 2, -1e-3))
    assert call(K=1) == (0, "")                                                     # a lone component
    assert call(w=0.0, K=0, a=None, b=None, c=None) == (0, "")                      # off, null pointers, K not looked at
    assert pp.evaluate(x)[0] == loss0
    # a refused call changes nothing: the last accepted mixture stays in force
    cfg = _set_gmm(packaged_config("video_mocap"), 1.0, 1.0)
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg, pose_mixture=mix)
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    l1 = p.evaluate(xc)[0]
    refused("1 .. 16 components", K=17)
    with torch.cuda.device(dev):
        from ctypes import byref

        from uuo_mocap_amd.engine import _ptr, current_stream

        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        grad = torch.empty((p.n,), dtype=torch.float32, device=dev)
        assert lib.uuo_closure_eval(p.fit, current_stream(dev), byref(p.problem), _ptr(xc), _ptr(loss), _ptr(grad), None) == 0
    assert float(loss.cpu()) == l1
    # lock-step batches
    assert p.pose_gmm_on
    with pytest.raises(NotImplementedError, match="lock-step.*pose_gmm"):
        solve_batch([p], [xc], max_iter=3)


# ------------------------------------------------------------------------------------------------ 7. the shipped configuration
def test_gmm_config(smpl, oracle_smpl, tables, dev, record_property):
    """A fit of the twisted-hip capture (120 x 30, seed 0) with video_mocap.yaml and with video_mocap_gmm.yaml: the shipped
    configuration runs on the fused closures end to end, its fit is finite, and the mean mixture energy of the fitted poses is
    not above the plain fit's.  The figures are reported (record_property); DESIGN 4z has the sweep at 300 x 50."""
    from uuo_mocap_amd.metrics import compute_pose_gmm_energy
    from uuo_mocap_amd.multimodal import multimodal_video_mocap
    from uuo_mocap_amd.synthetic import pose_mixture

    seq = make_sequence(tables, seed=0, num_frames=120, num_markers=30, pose_outlier=True)
    t0, t1 = seq.gt["outlier_window"]
    truth = torch.from_numpy(seq.gt["rot"][:, 1]).double()
    res = {}
    for name in ("video_mocap", "video_mocap_gmm"):
        cfg = packaged_config(name)
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 40
        out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0),
                                     dev, cfg, offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
        rot = torch.as_tensor(out["pose_body"]).cpu().double()
        assert torch.isfinite(rot).all()
        rel = truth.transpose(1, 2) @ rot[:, 0]
        err = torch.arccos((0.5 * (rel.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0)).clamp(-1.0, 1.0))
        r = oracle_smpl(torch.as_tensor(out["pose_body"]).cpu().float(), torch.as_tensor(out["betas"]).cpu().float(),
                        torch.as_tensor(out["root_orient"]).cpu().float(), torch.as_tensor(out["trans"]).cpu().float())
        res[name] = (compute_pose_gmm_energy(rot.float(), pose_mixture())["mean"], float(err[t0:t1].mean()),
                     float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean()))
        for key, v in zip(("energy", "window_joint1_rad", "vertex_m"), res[name]):
            record_property("%s_%s" % (name, key), v)
        print("OBS pose gmm config %s: mean energy %.3f, window joint-1 error %.4f rad, vertex error %.2f mm"
              % (name, res[name][0], res[name][1], 1e3 * res[name][2]))
    assert res["video_mocap_gmm"][0] <= res["video_mocap"][0]
