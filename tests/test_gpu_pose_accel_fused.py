"""EXTENSION: the pose-acceleration term on the fused chamfer and marker closures (execution.pose_accel_fused: True; k_pose_accel,
uuo_fit_set_pose_accel) on the MI355X: the term alone against float64 next to the composed fp32 term's own error, the whole
closures against float64 autograd, the buffer it shares with the joint-angle limit term and the weighted pose prior, off is off,
four evaluations in flight bit for bit (both stages), fused against composed solves, the library's refusals, and
video_mocap_rotsmooth_fused.yaml on the default capture."""
import copy
import ctypes
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pose_accel_ref64 import pose_accel_grad64, random_raw  # noqa: E402
from floor_ref64 import _contacts, _vids  # noqa: E402
from gpu_support import (R_CHAMFER, R_MARKER, U_TABLE, W_LIM_C, W_LIM_M, W_PACC_C as W_C, W_PACC_M as W_M, _inputs,  # noqa: E402,F401
                         _rel_err, dev, smpl, smpl64)
from joint_limits_ref64 import _block as _lim_block, _lim_grad, _preconditions as _lim_preconditions, _tables as _lim_tables  # noqa: E402
from prior_confidence_ref64 import _prior64, _weight_tables  # noqa: E402
from stage_ref64 import (_chamfer_forward64, _float64, _marker_forward64, ref_chamfer64 as _ref_chamfer,  # noqa: E402
                         ref_marker64 as _ref_marker)
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.metrics import LEAF_JOINT_ROWS  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 11


def _cfg(w_chamfer=None, w_marker=None, u=None, fused=True, limits=None, reg=None):
    """video_mocap.yaml with the term's key (None = absent) and joint weights, execution.pose_accel_fused, the joint-angle limit
    term on a table `limits`, and reg_pose_body `reg` = (chamfer, marker).  (floor_height: the stage reference
    reads it.)"""
    cfg = packaged_config("video_mocap")
    if fused:
        cfg["execution"] = dict(cfg.get("execution") or {}, pose_accel_fused=True)
    for i, (stage, w) in enumerate((("chamfer", w_chamfer), ("marker", w_marker))):
        st = cfg["stages"][stage]
        st["floor_height"] = 0.0
        if w is not None:
            st["losses"]["pose_accel"] = w
            if u is not None:
                st["pose_accel"] = {"joint_weights": list(u)}
        if limits is not None:
            st["losses"]["joint_limits"] = (W_LIM_C, W_LIM_M)[i]
            st["joint_limits"] = _lim_block(limits)
        if reg is not None:
            st["losses"]["reg_pose_body"] = reg[i]
    return cfg


def _alone(cfg):
    """no data term, no priors: loss and gradient ARE the extension terms"""
    cfg["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_pose_body=0.0, reg_betas=0.0)
    cfg["stages"]["marker"]["losses"].update(marker=0.0, reg_pose_body=0.0, reg_betas=0.0)
    return cfg


class _Case:
    """One (F, seed): the inputs, and per stage a maker of problems and the packed evaluation point with body pose `pose`
    (default: the perturbed pose of _inputs)."""

    def __init__(self, smpl, tables, dev, F, seed, num_markers=M):
        self.F, self.seed, self.smpl, self.dev = F, seed, smpl, dev
        seq, self.markers, self.o_pose, self.o_betas, self.root, self.trans, self.pert = _inputs(tables, F, seed, num_markers=num_markers)
        self.vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
        self.contacts = _contacts(F, seed)
        self.svids = _vids(tables, 6)
        self.pose_slice = {"chamfer": slice(4 * F + 10, 211 * F + 10), "marker": slice(0, 207 * F)}

    def make(self, stage, cfg, **kw):
        from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

        d = self.dev
        if stage == "chamfer":
            return ChamferProblem(self.smpl, self.markers.to(d), self.o_pose.to(d), self.o_betas.to(d), self.root.to(d), cfg, **kw)
        return MarkerProblem(self.smpl, self.markers.to(d), self.o_pose.to(d), self.o_betas.to(d), self.vids.to(d), cfg, **kw)

    def x(self, stage, prob, pose=None):
        tp, zp, bp, pp, rp = self.pert
        pose = pp if pose is None else pose
        d = self.dev
        if stage == "chamfer":
            return prob.pack(tp.to(d), zp.to(d), bp.to(d), pose.to(d))
        return prob.pack(pose.to(d), bp.to(d), rp.to(d), tp.to(d))

    def raw(self, stage, x):
        return x.detach().cpu()[self.pose_slice[stage]].reshape(self.F, 23, 3, 3)

    def term64(self, stage, x, w, u=None):
        """float64 loss and flat gradient (numpy, the closure's packing) of the term at x"""
        loss, g = pose_accel_grad64(self.raw(stage, x), w, u)
        out = np.zeros(x.numel())
        out[self.pose_slice[stage]] = g.reshape(-1).numpy()
        return loss, out

    def rest64(self, stage, smpl64, tables, cfg, x, nn=None):
        """float64 loss and gradient of the closure of `cfg` without the extension terms of this file (the stage reference)"""
        if stage == "chamfer":
            return _ref_chamfer(smpl64, cfg, self.markers, self.o_pose, self.o_betas, self.root, x, nn, self.contacts, self.svids, 3)
        return _ref_marker(smpl64, tables, cfg, self.markers, self.o_pose, self.o_betas, x, self.vids, None, self.contacts,
                           self.svids, 3, M)

    def leaves64(self, stage, smpl64, x):
        with _float64():
            if stage == "chamfer":
                return _chamfer_forward64(smpl64, x.detach().cpu().double(), self.root.double(), self.F)[0], 3
            return _marker_forward64(smpl64, x.detach().cpu().double()[:219 * self.F + 10], self.F)[0], 0


def _max_err(g, g64):
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def _composed32(raw, w, u):
    """the composed closures' term (losses.pose_accel_loss on normalize_rot of the raw entries) through float32 autograd"""
    from uuo_mocap_amd.losses import pose_accel_loss
    from uuo_mocap_amd.transforms import normalize_rot

    leaf = raw.detach().float().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(pose_accel_loss(normalize_rot(leaf), w, u), [leaf])
    return g.double().reshape(-1).numpy()


# ------------------------------------------------------------------------------------------------ 1. the term alone
def test_the_term_alone_against_float64_and_the_composed_term(smpl, tables, dev, record_property):
    """Chamfer and marker stage, F in {3, 4, 5, 33} (one a_t with every boundary case; the first interior frame; an odd F whose last
    block has an idle upper half), M = 11, ones and a joint-weight table with a zero, on pose_accel_ref64.random_raw poses (rows
    neither unit nor orthogonal).  With w_data = 0 and both priors 0 the closure IS the term; the term is the closure with the key
    on minus the closure at weight 0 at the same point (every other weight is 0 there, so the difference loses nothing).  Error:
    max|g - g64| / max|g64| against pose_accel_grad64.  The bound is the composed fp32 term's own error on the same inputs
    (losses.pose_accel_loss through float32 autograd): the fused error of every case stays within 8 x the largest composed error
    over the cases -- a wrong stencil coefficient or boundary gives O(1).  The loss: rtol 2e-5, the project's loss tolerance.
    Measured on the MI355X: see the two recorded properties (DESIGN 4v lists them)."""
    fused, composed = {}, {}
    for F in (3, 4, 5, 33):
        case = _Case(smpl, tables, dev, F, 500 + F)
        pose = random_raw(F, 40 + F)
        for u in (None, U_TABLE):
            g64 = None
            for stage in ("chamfer", "marker"):
                on = case.make(stage, _alone(_cfg(W_C, W_M, u)))
                off = case.make(stage, _alone(_cfg(0.0, 0.0, u)))
                assert on.pose_accel_on and not off.pose_accel_on
                x = case.x(stage, on, pose)
                l_on, g_on, _ = on.evaluate(x, want_nn=False)
                l_off, g_off, _ = off.evaluate(x, want_nn=False)
                l64, g64 = case.term64(stage, x, W_C, u)
                tag = (stage, F, "table" if u else "ones")
                fused[tag] = _max_err((g_on - g_off).cpu().double().numpy(), g64)
                np.testing.assert_allclose(l_on - l_off, l64, rtol=2e-5, err_msg=str(tag))
            raw = case.raw("marker", x)
            composed[(F, "table" if u else "ones")] = _max_err(_composed32(raw, W_C, u), g64[case.pose_slice["marker"]])
    worst_f, worst_c = max(fused.values()), max(composed.values())
    record_property("fused_max_error", worst_f)
    record_property("composed_fp32_max_error", worst_c)
    print("OBS pose accel fused, the term alone: fused max error %.3e, composed fp32 max error %.3e; per case fused %s composed %s"
          % (worst_f, worst_c, {k: "%.2e" % v for k, v in fused.items()}, {k: "%.2e" % v for k, v in composed.items()}))
    assert worst_c > 0.0
    for tag, err in fused.items():
        assert err <= 8.0 * worst_c, (tag, err, worst_c)


# ------------------------------------------------------------------------------------------------ 2. whole closures
@pytest.mark.parametrize("F", [5, 33])
def test_closures_match_float64_autograd(smpl, smpl64, tables, dev, F):
    """video_mocap.yaml plus the term at 1000 / 1000 with the joint-weight table, both stages: loss rtol 2e-5, gradient relative
    error < 2e-4 against float64 autograd (test_gpu_floor's restatement of the closures plus the term's own), and the term
    changes the gradient by more than 2e-2 relative (test_gpu_joint_limits' tolerances and precondition)."""
    case = _Case(smpl, tables, dev, F, 640 + F)
    cfg, cfg0 = _cfg(W_C, W_M, U_TABLE), _cfg()
    for stage, w in (("chamfer", W_C), ("marker", W_M)):
        prob, prob0 = case.make(stage, cfg), case.make(stage, cfg0)
        assert prob.pose_accel_on and prob.pacc_w == w and not prob0.pose_accel_on
        x = case.x(stage, prob)
        loss, grad, nn = prob.evaluate(x)
        _, grad0, nn0 = prob0.evaluate(x)
        if stage == "chamfer":
            assert torch.equal(nn, nn0), "the term must not change the assignment"
        l0, g0 = case.rest64(stage, smpl64, tables, cfg0, x, nn)
        lt, gt = case.term64(stage, x, w, U_TABLE)
        g = grad.cpu().numpy()
        share = _rel_err(g, grad0.cpu().numpy())
        print("OBS pose accel fused parity (%s, F %d): loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
              % (stage, F, abs(loss - (l0 + lt)) / abs(l0 + lt), _rel_err(g, g0 + gt), share))
        np.testing.assert_allclose(loss, l0 + lt, rtol=2e-5, err_msg=stage)
        assert _rel_err(g, g0 + gt) < 2e-4, stage
        assert share > 2e-2, stage


# ------------------------------------------------------------------------------------------------ 3. the shared buffer
@pytest.mark.parametrize("limits,prior", [(True, False), (False, True), (True, True)])
def test_the_buffer_shared_with_the_limit_term_and_the_weighted_prior(smpl, smpl64, tables, dev, limits, prior):
    """The term with joint_limits (+-0.2 rad on every component), with prior_confidence (hash weights with exact zeros, at
    test_gpu_prior_confidence's reg_pose_body), and with both -- the add chain k_limit_fwd -> k_pose_accel -> k_prior_conf through
    one buffer -- against float64 at the same tolerances, both stages, F = 7.  And a zero joint weight leaves the rows of that
    joint bitwise what they are with the same settings and no key."""
    F, seed = 7, 7870   # (test_gpu_joint_limits' seed for (7, 11): its preconditions hold)
    case = _Case(smpl, tables, dev, F, seed)
    tab = _lim_tables()["full"]
    if limits:
        _lim_preconditions(case.pert[3], tab[0], tab[1], 3)
    wtab = _weight_tables(F, seed)["hash"] if prior else None
    reg = (R_CHAMFER, R_MARKER) if prior else None
    kw = dict(limits=tab if limits else None, reg=reg)
    cfg, cfg0 = _cfg(W_C, W_M, U_TABLE, **kw), _cfg(**kw)
    rest = copy.deepcopy(cfg0)     # what test_gpu_floor's restatement covers: no limit term, and with weights no pose prior
    if prior:
        for stage in ("chamfer", "marker"):
            rest["stages"][stage]["losses"]["reg_pose_body"] = 0.0
    for i, (stage, w) in enumerate((("chamfer", W_C), ("marker", W_M))):
        prob, prob0 = case.make(stage, cfg, prior_weights=wtab), case.make(stage, cfg0, prior_weights=wtab)
        assert prob.pose_accel_on and prob.joint_limits_on == limits and prob.prior_conf_on == prior and not prob0.pose_accel_on
        x = case.x(stage, prob)
        loss, grad, nn = prob.evaluate(x)
        _, grad0, _ = prob0.evaluate(x)
        lo, g_ref = case.rest64(stage, smpl64, tables, rest, x, nn)
        if limits:
            leaves, pose_index = case.leaves64(stage, smpl64, x)
            ll, gl = _lim_grad(leaves, pose_index, tab, (W_LIM_C, W_LIM_M)[i])
            lo, g_ref = lo + ll, g_ref + gl
        if prior:
            lp, gp = _prior64(x, case.pose_slice[stage], case.o_pose, wtab, reg[i], x.numel())
            lo, g_ref = lo + lp, g_ref + gp
        lt, gt = case.term64(stage, x, w, U_TABLE)
        lo, g_ref = lo + lt, g_ref + gt
        g = grad.cpu().numpy()
        print("OBS pose accel fused shared buffer (%s, limits %s, prior %s): loss rel %.2e, gradient rel %.2e"
              % (stage, limits, prior, abs(loss - lo) / abs(lo), _rel_err(g, g_ref)))
        np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=stage)
        assert _rel_err(g, g_ref) < 2e-4, stage
        rows = lambda v: case.raw(stage, v)[:, 3]      # U_TABLE[3] == 0: SMPL joint 4
        assert torch.equal(rows(grad), rows(grad0)), stage
        assert not torch.equal(case.raw(stage, grad)[:, 9], case.raw(stage, grad0)[:, 9]), stage


def test_the_add_chains_of_both_shared_buffers_for_every_subset(smpl, smpl64, tables, dev):
    """The first kernel of an evaluation to reach a shared buffer writes it and the later ones add: lim_g takes k_limit_fwd,
    k_pose_accel and k_prior_conf, cap_up takes k_capsule_fwd and k_keypoint2d_fwd.  Marker stage, F = 5 (odd: the last 64-thread
    block has an idle half; the smallest F with an interior frame of k_pose_accel's five-frame stencil), M = 12.  Every one of the
    8 subsets of {limits, pose acceleration, weighted prior} crossed with the 4 of {capsules, key points} is evaluated on ONE
    workspace, one after another, in an order in which the last evaluation that wrote a buffer left it with another subset's
    contents (asserted), and on a fresh thread's workspace that has only ever seen that subset.  Loss and gradient are bitwise
    equal between the two workspaces and on a repeated evaluation: a kernel that adds where no earlier writer ran picks up the
    previous subset's contents, one that writes where it should add loses a term -- and the 32 losses are all different."""
    from keypoints2d_ref64 import evidence
    from capsules_ref64 import _block as _cap_block, _joints64, _lists as _cap_lists, _preconditions as _caps_preconditions
    from gpu_support import W_CAPS_M
    from uuo_mocap_amd.engine import set_workspace_slot

    F, markers, seed = 5, 12, 5120
    case = _Case(smpl, tables, dev, F, seed, num_markers=markers)
    lim_tab, cap_list, wtab = _lim_tables()["full"], _cap_lists(tables)["builder"], _weight_tables(F, seed)["hash"]
    joints = _joints64(smpl64, tables, F, markers, seed)[1]
    # every term is active at the evaluated point (host-side, float64)
    _lim_preconditions(case.pert[3], lim_tab[0], lim_tab[1], 1)
    _caps_preconditions(joints, cap_list, 1)
    rec = {k: v.float() for k, v in evidence(joints, seed).items()}

    def problem(limits, pose_accel, prior, caps, kp):
        cfg = _cfg(W_C if pose_accel else None, W_M if pose_accel else None, U_TABLE, limits=lim_tab if limits else None,
                   reg=(R_CHAMFER, R_MARKER))
        for stage in ("chamfer", "marker"):
            st = cfg["stages"][stage]
            if caps:
                st["losses"]["self_penetration"] = W_CAPS_M
                st["capsules"] = _cap_block(cap_list)
            if kp:
                st["losses"]["keypoints_2d"] = 0.02    # test_gpu_keypoints2d's weight, sigma and least depth
                st["keypoints_2d"] = {"sigma": 8.0, "min_depth": 0.1, "joint_weights": None}
        p = case.make("marker", cfg, prior_weights=wtab if prior else None, keypoints_2d=rec if kp else None)
        assert (p.joint_limits_on, p.pose_accel_on, p.prior_conf_on, p.capsules_on, p.keypoints_on) == \
            (limits, pose_accel, prior, caps, kp)
        return p

    flags = lambda lim, cap: (bool(lim & 1), bool(lim & 2), bool(lim & 4), bool(cap & 1), bool(cap & 2))
    lim_order, cap_order = (7, 1, 6, 2, 5, 3, 4, 0), (3, 1, 2, 0)
    order = [(lim_order[k % 8], cap_order[(k % 8 + k // 8) % 4]) for k in range(32)]
    assert len(set(order)) == 32
    x = case.x("marker", problem(*flags(0, 0)))
    shared, fresh = {}, {}
    left = [0, 0]    # the subsets whose contents lim_g and cap_up hold
    for lim, cap in order:
        assert (lim == 0 or lim != left[0]) and (cap == 0 or cap != left[1]), (lim, cap, left)
        left = [lim or left[0], cap or left[1]]
        p = problem(*flags(lim, cap))
        l1, g1, _ = p.evaluate(x, want_nn=False)
        l2, g2, _ = p.evaluate(x, want_nn=False)
        assert l1 == l2 and torch.equal(g1, g2), (lim, cap)
        shared[lim, cap] = (l1, g1)

    def on_fresh_workspace(k, lim, cap):
        set_workspace_slot(24 + k)
        fresh[lim, cap] = problem(*flags(lim, cap)).evaluate(x, want_nn=False)[:2]
        torch.cuda.synchronize()

    for k, (lim, cap) in enumerate(order):
        t = threading.Thread(target=on_fresh_workspace, args=(k, lim, cap))
        t.start()
        t.join()
    for key in order:
        assert key in fresh, key
        assert fresh[key][0] == shared[key][0] and torch.equal(fresh[key][1], shared[key][1]), key
    assert len({loss for loss, _ in shared.values()}) == 32


# ------------------------------------------------------------------------------------------------ 4. off is off
def test_off_is_off_and_on_is_deterministic(smpl, tables, dev):
    """Weight 0 (F = 9), and a positive weight at F = 2 (the term has no terms: no kernel runs), are bitwise the config without
    the key, on a workspace that has just run with the term on; third rows of the pose gradient of the term alone are exact zeros;
    two evaluations, and two fresh threads that run at the same time (each on a workspace slot of its own, beside a third that
    runs the plain closure), give bitwise equal results."""
    for F in (9, 2):
        case = _Case(smpl, tables, dev, F, 313 + F)
        for stage in ("chamfer", "marker"):
            absent, zero, on = _cfg(fused=False), _cfg(0.0, 0.0, U_TABLE), _cfg(W_C, W_M, U_TABLE)
            p0, pz, pw = case.make(stage, absent), case.make(stage, zero), case.make(stage, on)
            assert pw.pose_accel_on and not pz.pose_accel_on and not p0.pose_accel_on
            x = case.x(stage, pw)
            fresh = {}

            def on_fresh_thread(key, cfg, slot):  # a workspace belongs to a slot: each thread takes one of its own
                from uuo_mocap_amd.engine import set_workspace_slot

                set_workspace_slot(slot)
                p = case.make(stage, cfg)
                fresh[key] = p.evaluate(x, want_nn=False)[:2]
                torch.cuda.synchronize()

            threads = [threading.Thread(target=on_fresh_thread, args=a) for a in (("plain", absent, 5), ("on a", on, 6), ("on b", on, 7))]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            lf, gf = fresh["plain"]
            lw, gw, _ = pw.evaluate(x, want_nn=False)
            lw2, gw2, _ = pw.evaluate(x, want_nn=False)
            assert lw == lw2 and torch.equal(gw, gw2), (F, stage)
            for key in ("on a", "on b"):
                assert fresh[key][0] == lw and torch.equal(fresh[key][1], gw), (F, stage, key)
            if F == 2:
                assert lw == lf and torch.equal(gw, gf), stage       # a positive weight at F = 2: the key absent, bit for bit
            else:
                assert lw > lf and not torch.equal(gw, gf), stage
            for tag, p in (("absent", p0), ("weight 0", pz)):
                pw.evaluate(x, want_nn=False)                          # the workspace has just run with the term on
                l0, g0, _ = p.evaluate(x, want_nn=False)
                assert l0 == lf and torch.equal(g0, gf), (F, stage, tag)
            if F > 2:
                alone = case.make(stage, _alone(_cfg(W_C, W_M, U_TABLE)))
                _, ga, _ = alone.evaluate(x, want_nn=False)
                pg = case.raw(stage, ga)
                assert bool(pg[:, :, :2].any()) and not bool(pg[:, :, 2].any()), stage


# ------------------------------------------------------------------------------------------------ 5. four in flight
@pytest.mark.parametrize("stage", ["marker", "chamfer"])
def test_four_in_flight_are_bit_identical_to_one(smpl, tables, dev, stage, record_property):
    """parallel.fit_many over 8 problems at F = 33, 30 evaluations each at perturbed points (test_gpu_keypoints2d's shape): every
    loss and gradient with inflight=4 is bitwise equal to the same work with inflight=1 -- 240 evaluations per stage.  The chamfer
    stage is where the first k_pose_accel had 29 wrong of 600."""
    from uuo_mocap_amd.parallel import fit_many

    F, N, E = 33, 8, 30
    cfg = _cfg(W_C, W_M, U_TABLE)
    items = [_Case(smpl, tables, dev, F, 400 + i) for i in range(N)]

    def work(case):
        p = case.make(stage, cfg)
        assert p.pose_accel_on
        x0 = case.x(stage, p)
        gen = torch.Generator().manual_seed(case.seed)
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


# ------------------------------------------------------------------------------------------------ 6. fused vs composed
def test_fused_and_composed_pose_accel_solves_agree(smpl, tables, dev):
    """10 L-BFGS iterations of the chamfer and the marker stage at F = 9 on the fused closures (execution.pose_accel_fused: True)
    and on the operator-composed ones (the switch absent): the start agrees to 1e-5, the end to 5e-2 / 8e-2
    (test_fused_and_composed_keypoint_solves_agree's tolerances), and both decrease."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F, num_markers=M)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    out = {}
    for fused in (True, False):
        cfg = _cfg(W_C, W_M, U_TABLE, fused=fused)
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 10
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
    assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf and "first_loss" in mf   # (the routes' statistics)
    print("OBS pose accel fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (F, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=8e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)
    assert final(cc) < first(cc) and final(mc) < first(mc)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_library_refuses_the_term_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103, num_markers=M)
    md = markers.to(dev)

    def arm(p, w=1.0):  # what no config can produce: the library itself must refuse it
        p.pacc_w, p.pacc_u = w, None

    # the part stage refuses at evaluation
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    arm(pp)
    with pytest.raises(RuntimeError, match="pose-acceleration term.*part stage"):
        pp.evaluate(x)
    arm(pp, 0.0)
    assert pp.evaluate(x)[0] == loss0
    # the soft chamfer closure refuses at evaluation, and its problem at construction
    soft = packaged_config("video_mocap")
    soft["stages"]["chamfer"]["losses"]["soft_chamfer"] = 10.0
    ps = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft)
    xs = ps.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    ls0 = ps.evaluate(xs)[0]
    arm(ps)
    with pytest.raises(RuntimeError, match="pose-acceleration term.*soft-assignment"):
        ps.evaluate(xs)
    arm(ps, 0.0)
    assert ps.evaluate(xs)[0] == ls0
    soft_on = copy.deepcopy(soft)
    soft_on["execution"] = {"pose_accel_fused": True}
    soft_on["stages"]["chamfer"]["losses"]["pose_accel"] = 1.0
    with pytest.raises(NotImplementedError, match="pose_accel.*soft-assignment closure"):
        ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft_on)
    # the setter: every bad weight and table entry; null = ones; off looks at nothing
    lib, fit = smpl.device_model.lib, pp.fit
    cf = ctypes.c_float
    good = np.ascontiguousarray(np.asarray(U_TABLE, dtype=np.float32))

    def call(w=1.0, table=good, fit=fit):
        return lib.uuo_fit_set_pose_accel(fit, cf(w), None if table is None else table.ctypes.data)

    assert call() == 0 and call(table=None) == 0 and call() == 0
    assert call(fit=None) == -22
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(w=bad) == -22, bad
        t = good.copy()
        t[5] = bad
        assert call(table=t) == -22, bad
        assert b"joint weight" in lib.uuo_last_error()
    assert call(w=0.0, table=None) == 0   # off: nothing else is looked at
    assert pp.evaluate(x)[0] == loss0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), _cfg(1.0, 1.0))
    assert p.pose_accel_on
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step.*pose_accel"):
        solve_batch([p], [xc], max_iter=3)


# ------------------------------------------------------------------------------------------------ 8. the shipped config
def test_rotsmooth_fused_config(smpl, tables, dev, record_property):
    """Default 300 x 50 synthetic capture (seed 0), fitted with video_mocap.yaml and with video_mocap_rotsmooth_fused.yaml: the
    leaf-joint rotation-acceleration error of the new config is below the plain config's (an ordering; the composed fit's recorded
    gap is three orders of magnitude: 458.8 -> 0.126).  The figures and the fit's wall time are recorded; no equality with the
    composed fit is asserted, since the trajectories differ."""
    import time

    from uuo_mocap_amd.metrics import compute_rotation_accel_error
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50)
    gt_rot = torch.from_numpy(np.asarray(seq.gt["rot"]))[:, 1:].double()
    res = {}
    for name in ("video_mocap", "video_mocap_rotsmooth_fused"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0),
                                     dev, packaged_config(name), offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
        torch.cuda.synchronize()
        rot = out["pose_body"].cpu().double()
        res[name] = {"leaf": float(compute_rotation_accel_error(rot, gt_rot, 30.0, LEAF_JOINT_ROWS)),
                     "all": float(compute_rotation_accel_error(rot, gt_rot, 30.0)), "seconds": time.perf_counter() - t0}
        for k, v in res[name].items():
            record_property("%s_%s" % (name, k), v)
    a, b = res["video_mocap"], res["video_mocap_rotsmooth_fused"]
    print("OBS pose accel fused (default capture): rotation-acceleration error leaf %.3f -> %.3f, all %.3f -> %.3f; fits %.2f s, "
          "%.2f s" % (a["leaf"], b["leaf"], a["all"], b["all"], a["seconds"], b["seconds"]))
    assert b["leaf"] < a["leaf"], res
