"""The fused 2D-prior closure (uuo_reprojection_eval; k_reproj_search, k_reproj_terms, k_reproj_sum of csrc/reprojection.hip)
on the MI355X against float64 at the sizes where its code changes path, on small synthetic clouds fed straight to
engine.ReprojectionProblem (no SMPL forward).  The yardstick is tests/reprojection_ref64.py, the reference's formulation
under float64 autograd, pinned to the oracle by tests/test_reprojection_reference.py.

(a) exact ties on a lattice: the four merges of the search (lane, wave butterfly, 4 waves, 4 slices) keep the first index;
(b) the search on random clouds: every index is the float64 argmin, or a vertex within the fp32 rounding of it;
(c) loss, gradient (whole and per parameter block) and key points, fractional and zero masks, either term alone;
(d) the Python surface with invalid HMR frames against the oracle;
(e) markers without a minimum (NaN): no contribution, index -1.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reprojection_ref64 as rr  # noqa: E402
from gpu_support import dev, smpl  # noqa: E402,F401

from oracle import stages_ref  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import ReprojectionProblem  # noqa: E402

LOSS_RTOL, GRAD_REL, BLOCK_REL, KP_ATOL = 2e-5, 2e-4, 5e-4, 2e-5  # test_gpu_fullsize's; _check_grad's; the fixture test's


def _device_eval(case, dev):
    """(loss, grad, kp, nn) of the library at the case's point; the evaluation is repeated and must not change by a bit."""
    d = lambda k: torch.from_numpy(case[k]).to(dev)
    prob = ReprojectionProblem(d("markers"), d("joints0"), d("verts0"), d("kp_target"), d("mask"), case["focal"],
                               case["centre"], case["w_reprojection"], case["w_chamfer"])
    assert prob.n == 3 * case["F"] + 14
    x = d("x").contiguous()
    loss, grad, kp, nn = prob.evaluate(x, want_kp=True, want_nn=True)
    loss2, grad2, _, nn2 = prob.evaluate(x, want_kp=True, want_nn=True)
    grad, kp, nn = grad.cpu().numpy(), kp.cpu().numpy(), nn.cpu().numpy()
    same = np.float32(loss).tobytes() == np.float32(loss2).tobytes() and grad.tobytes() == grad2.cpu().numpy().tobytes() \
        and np.array_equal(nn, nn2.cpu().numpy())
    return dict(loss=loss, grad=grad, kp=kp, nn=nn, repeatable=same)


_CACHE = {}


def _evaluated(key, build, dev):
    """The case of `key`, the library's evaluation of it and the float64 evaluation (at its own argmin): computed once per
    session and shared by the search and the closure test."""
    if key not in _CACHE:
        case = build()
        out = _device_eval(case, dev)
        out["case"] = case
        out["ref"] = rr.evaluate(case)
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ (a) exact lattice ties
@pytest.mark.parametrize("M", [16, 17, 33, 50, 65])
@pytest.mark.parametrize("V", [1029, 6890])
def test_lattice_ties_keep_the_first_index(dev, V, M):
    """Dyadic coordinates, yaw = 0, b = 0, j0 = 0: every fp32 operation of the search is exact, and every marker's minimum is
    attained by two (or four) vertices whose indices straddle one merge -- the same lane (i, i + 256), neighbouring lanes
    (i, i + 1), two waves (i, i + 64), two, or all four, slices -- planted as duplicates and as mirror images, for every
    marker of every register pass (rr.lattice_case).  The table must equal the lowest index of the integer minimum."""
    case, expected, planted, _ = rr.lattice_case(V, M)
    out = _device_eval(case, dev)
    wrong = np.argwhere(out["nn"] != expected)
    msg = "; ".join("frame %d marker %d (%s): %d, expected %d" % (f, m, rr.LATTICE_KINDS[planted[f, m]] if planted[f, m] >= 0
                                                                    else "no plant", out["nn"][f, m], expected[f, m])
                    for f, m in wrong[:8])
    assert len(wrong) == 0, "%d of %d indices differ: %s" % (len(wrong), expected.size, msg)
    assert out["repeatable"]


# ------------------------------------------------------------------------------------------------ (b) the search
def _search_key(F, M, V, yi):
    return ("search", F, M, V, yi)


def _check_search(res, tag, record_property):
    """Every index is the float64 argmin; a pair whose float64 gap between the best and the second-best vertex is below the
    fp32 rounding bound of the two distances (rr.d2_rounding_bound: derived from u = 2^-24 and the case's magnitudes) may
    name another vertex, which must then be within that bound of the minimum.  At most 1 % of a case's pairs are such."""
    case, nn = res["case"], res["nn"]
    _, _, _, d2, nn64 = res["ref"]
    assert nn.shape == nn64.shape and nn.min() >= 0 and nn.max() < case["V"], (tag, int(nn.min()), int(nn.max()))
    bound, left = rr.left_out(case, d2)
    share = float(left.mean())
    record_property("left_out_share_%s" % tag, share)
    assert share < 0.01, (tag, share)
    differs = nn != nn64
    assert not (differs & ~left).any(), "%s: %d indices off the float64 argmin on pairs that are no near-tie: %s" % (
        tag, int((differs & ~left).sum()), np.argwhere(differs & ~left)[:8].tolist())
    excess = np.take_along_axis(d2, nn[..., None].astype(np.int64), -1)[..., 0] - d2.min(-1)
    assert (excess[left] <= bound[left]).all(), (tag, float(excess[left].max()))
    return share, int(differs.sum())


@pytest.mark.parametrize("F,M,V", rr.SEARCH_CASES, ids=lambda v: str(v))
def test_search_matches_float64_argmin(dev, record_property, F, M, V):
    for yi in range(len(rr.YAWS)):
        res = _evaluated(_search_key(F, M, V, yi), lambda: rr.search_case(F, M, V, yi), dev)
        share, flips = _check_search(res, "yaw%d" % yi, record_property)
        print("OBS reprojection search %dx%dx%d yaw %.2f: left out %.4f, %d indices off the float64 argmin"
              % (F, M, V, rr.YAWS[yi], share, flips))


# ------------------------------------------------------------------------------------------------ (c) the closure
def _block_err(g, g64, sl, total):
    """_check_grad's measure of a block: relative to its own float64 norm, or -- where that is below 1e-6 of the whole
    gradient's -- absolute in units of the whole gradient's norm."""
    e, n = float(np.linalg.norm(g[sl] - g64[sl])), float(np.linalg.norm(g64[sl]))
    return e / n if n >= 1e-6 * total else e / total


def _check_closure(res, tag, record_property, valid=None):
    """Loss rtol 2e-5, flat gradient rel-L2 < 2e-4, key points atol 2e-5 (image size 1) against float64 evaluated at the
    library's own assignment; every parameter block within max(5e-4, twice the error of the same restatement run in fp32 on
    the CPU); the detached betas' entries exactly 0; a repeated evaluation bit-identical."""
    case = res["case"]
    F = case["F"]
    assign = np.where(res["nn"] >= 0, res["nn"], 0)
    l64, g64, kp64, _, _ = rr.evaluate(case, assign=assign, valid=valid)
    l32, g32, _, _, _ = rr.evaluate(case, dtype=torch.float32, assign=assign, valid=valid)
    loss, grad = res["loss"], res["grad"].astype(np.float64)
    assert np.isfinite(loss) and np.isfinite(grad).all(), tag
    assert res["repeatable"], tag
    assert np.all(res["grad"][-10:] == 0.0), tag
    np.testing.assert_allclose(res["kp"], kp64, rtol=0, atol=KP_ATOL, err_msg=tag)
    total = float(np.linalg.norm(g64))
    if total == 0.0:  # nothing in the objective (no valid frame, no chamfer term)
        assert l64 == 0.0 and loss == 0.0 and not grad.any(), tag
        return {}
    whole = float(np.linalg.norm(grad - g64) / total)
    record_property("loss_rel_%s" % tag, abs(loss - l64) / abs(l64))
    record_property("grad_rel_%s" % tag, whole)
    msg, bad, errs = ["%s: loss %.8g (float64 %.8g), gradient %.2e" % (tag, loss, l64, whole)], [], {}
    for name, sl in rr.blocks(F):
        e_dev, e_32 = _block_err(grad, g64, sl, total), _block_err(g32.astype(np.float64), g64, sl, total)
        record_property("block_%s_%s_kernel" % (name, tag), e_dev)
        record_property("block_%s_%s_fp32" % (name, tag), e_32)
        msg.append("%s %.2e (fp32 torch %.2e)" % (name, e_dev, e_32))
        errs[name] = (e_dev, e_32)
        if not e_dev <= max(BLOCK_REL, 2.0 * e_32):
            bad.append(name)
    print("OBS reprojection closure " + "; ".join(msg))
    assert abs(loss - l64) <= LOSS_RTOL * abs(l64), "; ".join(msg)
    assert whole < GRAD_REL and not bad, "; ".join(msg) + " -- over the bar: %s" % bad
    return errs


# J: one lane, SMPL's 24, the fit's 45, the last lane but one and the full wave; masks: every frame invalid, and every value
# mean(cam_t == cam_t) can take (8 frames cycle through 0, 1/3, 2/3, 1); each term alone
EXTRA_CASES = [("J%d" % j, dict(F=2, M=17, V=255, J=j, yaw=rr.YAWS[i % 4], seed=20 + i)) for i, j in enumerate((1, 24, 45, 63, 64))] + [
    ("mask-all-zero", dict(F=3, M=17, V=255, yaw=-2.5, seed=30, mask=0.0)),
    ("mask-all-zero-no-chamfer", dict(F=3, M=17, V=255, yaw=-2.5, seed=30, mask=0.0, w_chamfer=0.0)),
    ("mask-fractions", dict(F=8, M=17, V=255, yaw=7.0, seed=31, mask="mixed")),
    ("mask-third", dict(F=1, M=17, V=255, yaw=0.0, seed=32, mask=1.0 / 3.0)),
    ("no-chamfer", dict(F=2, M=33, V=1025, yaw=np.pi / 2, seed=33, w_chamfer=0.0)),
    ("no-reprojection", dict(F=2, M=33, V=1025, yaw=-2.5, seed=34, w_reprojection=0.0)),
    ("weights", dict(F=2, M=33, V=1025, yaw=7.0, seed=35, w_reprojection=0.25, w_chamfer=30.0)),
]


@pytest.mark.parametrize("F,M,V", rr.SEARCH_CASES, ids=lambda v: str(v))
def test_closure_matches_float64_at_search_shapes(dev, record_property, F, M, V):
    for yi in range(len(rr.YAWS)):
        res = _evaluated(_search_key(F, M, V, yi), lambda: rr.search_case(F, M, V, yi), dev)
        _check_closure(res, "%dx%dx%d-yaw%d" % (F, M, V, yi), record_property)


@pytest.mark.parametrize("name,spec", EXTRA_CASES, ids=[n for n, _ in EXTRA_CASES])
def test_closure_matches_float64_joints_masks_weights(dev, record_property, name, spec):
    res = _evaluated(("extra", name), lambda: rr.random_case(**spec), dev)
    assert set(np.unique(res["case"]["mask"])) <= set(np.float32(rr.MASK_VALUES))
    if name == "mask-fractions":
        assert len(np.unique(res["case"]["mask"])) == 4
    _check_search(res, name, record_property)
    _check_closure(res, name, record_property)


# ------------------------------------------------------------------------------------------------ (d) the Python surface
def test_invalid_hmr_frames_through_the_python_surface(smpl, oracle_smpl, golden, dev):
    """reprojection_problem on the 8-frame fixture set-up with NaN in pred_cam on whole frames: the frame mask is 0 there, loss
    and gradient are finite and match the oracle's restatement of the reference closure (stages_ref.optim_reprojection, first
    evaluation) fed the same inputs, at the bars of the closure test."""
    from uuo_mocap_amd.reprojection import reprojection_problem

    g = golden("reprojection_stage.npz")
    cfg = packaged_config("video_mocap")
    t = lambda k: torch.from_numpy(np.asarray(g[k])).float()
    bad = [2, 5, 6]
    pred_cam = t("pred_cam")
    pred_cam[bad] = float("nan")
    for angle in (0.0, float(np.pi / 2)):
        args = dict(markers=t("markers"), pose_body=t("hmr_pose_body"), betas=t("betas"), hmr_betas=t("hmr_betas"),
                    root_orient=t("hmr_root_orient"), trans=t("trans"), pred_cam=pred_cam, cam_center=t("center"),
                    cam_size=t("size"), cam_scale=t("scale"), angle=torch.tensor(angle))
        cap = {}
        out = stages_ref.optim_reprojection(img_mask=t("img_mask"), smpl_inference=oracle_smpl, num_iters=1, config=cfg,
                                            capture=cap, **args)
        prob, x0 = reprojection_problem(smpl_inference=smpl, config=cfg,
                                        **{k: (v.to(dev) if v.dim() > 0 else v) for k, v in args.items()})
        mask = prob._keep[4].cpu().numpy()
        assert np.all(mask[bad] == 0.0) and np.all(np.delete(mask, bad) == 1.0)
        np.testing.assert_array_equal(mask, out["reproject_mask"].numpy())
        assert torch.isfinite(x0).all()
        np.testing.assert_allclose(x0.cpu().numpy(), cap["params"].numpy(), atol=3e-5)
        loss, grad, kp, nn = prob.evaluate(cap["params"].to(dev).contiguous(), want_kp=True, want_nn=True)
        grad = grad.cpu().numpy()
        assert np.isfinite(loss) and np.isfinite(grad).all() and torch.isfinite(kp).all()
        assert int(nn.min()) >= 0 and int(nn.max()) < 6890
        gref = cap["grad"].numpy()
        rel = float(np.linalg.norm(grad - gref) / np.linalg.norm(gref))
        print("OBS reprojection invalid frames yaw %.2f: loss %.6f (oracle %.6f), gradient rel-L2 %.2e"
              % (angle, loss, cap["loss"], rel))
        assert np.isfinite(cap["loss"]) and loss == pytest.approx(cap["loss"], rel=LOSS_RTOL)
        assert rel < GRAD_REL
        assert np.all(grad[1:25].reshape(8, 3)[bad] != 0.0)  # (the chamfer term still pulls the invalid frames' bodies)


# ------------------------------------------------------------------------------------------------ (e) markers without a minimum
def test_nan_markers_contribute_nothing_and_get_no_vertex(dev, record_property):
    """NaN markers in the first and in the (partial) last register pass, in both lane rounds of the terms kernel: the loss and
    the gradient equal float64 with those pairs removed and the divisor F M unchanged, and their nearest vertex is -1."""
    F, M, V = 2, 70, 1025
    holes = [(0, 3), (1, 15), (0, 66), (1, 69), (1, 40)]
    case = rr.random_case(F, M, V, yaw=-2.5, seed=40)
    valid = np.ones((F, M), bool)
    for f, m in holes:
        case["markers"][f, m, (f + m) % 3] = np.nan
        valid[f, m] = False
    case["markers"][0, 66] = np.nan
    out = _device_eval(case, dev)
    out["case"] = case
    nn = out["nn"]
    assert np.isfinite(out["loss"]) and np.isfinite(out["grad"]).all()
    # the other pairs: the search criterion of (b) on the float64 distances of the valid markers
    filled = dict(case, markers=np.where(valid[..., None], case["markers"], np.float32(0.0)))
    out["ref"] = rr.evaluate(filled)
    keep = dict(out, case=filled, nn=np.where(valid, nn, out["ref"][4]).astype(nn.dtype))
    assert (nn[valid] >= 0).all() and (nn[valid] < V).all()
    _check_search(keep, "nan-markers", record_property)
    _check_closure(out, "nan-markers", record_property, valid=valid)
    assert (nn[~valid] == -1).all(), nn[~valid]
