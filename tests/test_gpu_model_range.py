"""The fit kernels against float64 on the heavy-tailed stress model (tests/stress_model.py), loaded through
body_model.load_smpl_pkl: six decades of blend-basis magnitudes up to 0.2 m, fp16-subnormal basis entries, four skin
weights down to 1e-5, 100..300-entry joint-regressor rows.  Inputs: captures of make_sequence on that model at F = 300 and
at a ragged F = 17 (M = 50), whose marker positions are moved onto the stress body at the evaluation point; betas uniform in
[-5, 5]; identity, folded (hips, knees, shoulders, elbows bent by about pi - 0.3) and random full-range poses;
translations up to 3 m.

Bounds.  Forward vertices and joints: max |error| <= max(4 x the CPU float32 oracle's level, 1e-6 m) and <= 5e-6 m.  The
chamfer closure's fp16-split vertices: max <= max(1.25 x the fp32 kernel's max, 5e-7 m), mean <= 1.1 x its mean,
max <= 5e-6 m.  Gradients: the whole vector < 2e-4 relative (the suite's bar) and every parameter block < 5e-4 relative, or,
for a block whose float64 norm is below 1e-6 of the total, an absolute error below 5e-4 x the total norm.  Observed maxima
are recorded with record_property."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_model as sm  # noqa: E402

from gpu_support import _check_grad, dev  # noqa: E402,F401  (smpl and smpl64 are this file's own: the stress model's)
from oracle import p3d_ref  # noqa: E402
from stage_ref64 import _d64, _float64, ref_chamfer64, ref_marker64, ref_part64 as _ref_part  # noqa: E402,F401
from uuo_mocap_amd.body_model import hash_normal  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 50
CASES = [(300, 0), (17, 1)]  # (frames, seed)
VERT_CAP = 5e-6
# the stage references as this file calls them: the chamfer stage's without rho and with the float64 vertices, the marker stage's
# without latent offsets (no model tables needed)
_ref_chamfer = functools.partial(ref_chamfer64, sigma=0.0, with_vertices=True)


def _ref_marker(smpl64, cfg, *args):
    return ref_marker64(smpl64, None, cfg, *args)


@pytest.fixture(scope="module")
def pkl(tmp_path_factory):
    return sm.write_pkl(str(tmp_path_factory.mktemp("stress") / "SMPL_NEUTRAL.pkl"))


@pytest.fixture(scope="module")
def st(pkl):
    return sm.load(pkl)


@pytest.fixture(scope="module")
def smpl(st, dev):
    from uuo_mocap_amd.smpl import SmplInference

    return SmplInference(dev, tables=st)


@pytest.fixture(scope="module")
def smpl64(st):
    from oracle.smpl_ref import SmplInferenceRef

    return SmplInferenceRef(st).double()


def _rz64(z):
    """The rotation about z by each angle of `z` [F, 1, 1], in float64: [F, 1, 3, 3]."""
    ang = z.double().reshape(-1)
    r = torch.zeros(ang.shape[0], 1, 3, 3, dtype=torch.float64)
    r[:, 0, 0, 0], r[:, 0, 0, 1], r[:, 0, 1, 0], r[:, 0, 1, 1], r[:, 0, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1.0
    return r


# ------------------------------------------------------------------------------------------------ shared inputs
@pytest.fixture(scope="module")
def cases(st, smpl64):
    """Per (F, seed): the stress inputs, a make_sequence capture on the stress model (dropout pattern, marker vertex ids,
    HMR pose / betas as regulariser targets) and its markers moved onto the stress body at the evaluation point (root
    Rz(z) root, shared betas): 9.5 mm off the surface vertex with 1 cm of noise, so that the searches run among folded
    limbs."""
    out = {}
    for F, seed in CASES:
        inp = sm.stress_inputs(F, seed)
        seq = make_sequence(st, seed=seed, num_frames=F, num_markers=M)
        vids = np.asarray(seq.gt["marker_vids"]).astype(np.int64)
        root_eval = (_rz64(torch.from_numpy(inp["z"])) @ torch.from_numpy(inp["root"]).double()).float()
        with torch.no_grad():
            v = smpl64(*_d64(inp["pose"], np.repeat(inp["betas"], F, 0), root_eval, inp["trans"]))["vertices"].numpy()
        present = np.abs(np.nan_to_num(seq.markers.get_points())).sum(-1) != 0
        mk = v[:, vids] + 0.01 * hash_normal(977 + seed, F, M, 3)
        mk = np.where(present[..., None], mk, 0.0).astype(np.float32)
        o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float()
        out[F] = dict(inp=inp, seq=seq, vids=vids, markers=torch.from_numpy(mk), root_eval=root_eval,
                      o_pose=seq.img_smpl.pose_body.clone().float(), o_betas=o_betas)
    return out


@pytest.fixture(scope="module")
def fp32_level(st):
    """The CPU float32 oracle's max error against float64 on the forward inputs (tests/test_model_range.py prints it)."""
    lv = {}
    for F, seed in CASES:
        lv[F] = sm.forward_error(st, sm.stress_inputs(F, seed))
    return lv


# ------------------------------------------------------------------------------------------------ a. uuo_smpl_forward
@pytest.mark.parametrize("F", [F for F, _ in CASES])
def test_smpl_forward_against_float64(smpl, smpl64, cases, fp32_level, dev, record_property, F):
    """k_pose_prep + k_skin2 + k_joints45: vertices and the 45 joints (per-frame betas)."""
    inp = cases[F]["inp"]
    args = [torch.from_numpy(inp[k]) for k in ("pose", "betas_f", "root", "trans")]
    verts, joints = smpl.device_model.smpl_forward(*[a.to(dev) for a in args])
    with torch.no_grad():
        o = smpl64(*_d64(*args))
    ev = float(np.abs(verts.cpu().double().numpy() - o["vertices"].numpy()).max())
    ej = float(np.abs(joints.cpu().double().numpy() - o["joints"].numpy()).max())
    lv, lj = fp32_level[F]
    print("forward F=%d: vertices %.3e m (fp32 oracle %.3e), joints %.3e m (fp32 oracle %.3e)" % (F, ev, lv, ej, lj))
    record_property("forward_verts_max_abs_F%d" % F, ev)
    record_property("forward_joints_max_abs_F%d" % F, ej)
    assert ev <= max(4.0 * lv, 1e-6) and ev <= VERT_CAP
    assert ej <= max(4.0 * lj, 1e-6) and ej <= VERT_CAP


# ------------------------------------------------------------------------------------------------ b. chamfer closure


_CHAMFER_CHILD = """
import os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from uuo_mocap_amd import _lib
_lib.LIB_PATH = _lib.LIB_DEBUG_PATH  # the kernel-variant knob exists in the debug flavour only
import stress_model as sm
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.engine import ChamferProblem
from uuo_mocap_amd.smpl import SmplInference
dev = torch.device('cuda:0')
s = SmplInference(dev, tables=sm.load(%(pkl)r))
lib = _lib.load_debug()
out = {}
for F in %(frames)r:
    d = np.load(os.path.join(%(tmp)r, 'in%%d.npz' %% F))
    g = lambda k: torch.from_numpy(d[k]).to(dev)
    prob = ChamferProblem(s, g('markers'), g('o_pose'), g('o_betas'), g('root'), packaged_config('video_mocap'))
    x = prob.pack(g('t'), g('z'), g('b'), g('p'))
    for tag, on in (('f16', '1'), ('f32', '0')):
        os.environ['UUO_SKIN_F16'] = on
        loss, grad, nn = prob.evaluate(x)
        torch.cuda.synchronize()
        verts = np.zeros((F, 6890, 3), np.float32)
        bbox = np.zeros((F, 431, 6), np.float32)
        assert lib.uuo_debug_fit_buffers(prob.fit, verts.ctypes.data, bbox.ctypes.data) == 0
        out.update({'%%s_%%d_%%s' %% (tag, F, k): v for k, v in (('loss', loss), ('grad', grad.cpu().numpy()),
                    ('nn', nn.cpu().numpy()), ('verts', verts), ('bbox', bbox), ('x', x.cpu().numpy()))})
np.savez(os.path.join(%(tmp)r, 'out.npz'), **out)
"""


@pytest.fixture(scope="module")
def chamfer_runs(cases, pkl, tmp_path_factory):
    """One child process on the debug flavour (UUO_SKIN_F16=1: k_skin3, the default route; 0: the fp32 k_skin2) evaluates
    the chamfer closure at the stress point of every case and returns loss, gradient, assignment, the stored vertices and
    the unit boxes."""
    tmp = tmp_path_factory.mktemp("chamfer")
    for F, c in cases.items():
        inp = c["inp"]
        np.savez(tmp / ("in%d.npz" % F), markers=c["markers"].numpy(), o_pose=c["o_pose"].numpy(), o_betas=c["o_betas"].numpy(),
                 root=inp["root"], t=inp["trans"], z=inp["z"], b=inp["betas"], p=inp["pose"])
    code = _CHAMFER_CHILD % dict(root=ROOT, pkl=pkl, tmp=str(tmp), frames=[F for F, _ in CASES])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(tmp / "out.npz")


@pytest.mark.parametrize("F", [F for F, _ in CASES])
def test_chamfer_closure_default_route_against_float64(smpl64, cases, chamfer_runs, record_property, F):
    """k_skin3 -> unit boxes -> k_nn_cull -> k_bwd_sparse -> finalize: the fp16-split vertices against float64 (and against
    the fp32 kernel's distance to float64), the boxes exact, the assignment bit-equal to the CPU brute-force loop on the
    closure's own stored vertices in every frame, loss and gradient per block against float64 autograd."""
    c, o = cases[F], chamfer_runs
    inp = c["inp"]
    cfg = packaged_config("video_mocap")
    x = o["f16_%d_x" % F]
    nn = o["f16_%d_nn" % F].astype(np.int64)
    lo, g_ref, v64 = _ref_chamfer(smpl64, cfg, c["markers"], c["o_pose"], c["o_betas"], torch.from_numpy(inp["root"]), x, nn)
    # vertices
    e16 = np.abs(o["f16_%d_verts" % F].astype(np.float64) - v64)
    e32 = np.abs(o["f32_%d_verts" % F].astype(np.float64) - v64)
    print("chamfer F=%d vertices vs float64: fp16-split max %.3e mean %.3e; fp32 max %.3e mean %.3e"
          % (F, e16.max(), e16.mean(), e32.max(), e32.mean()))
    record_property("skin16_max_abs_F%d" % F, float(e16.max()))
    record_property("skin16_mean_abs_F%d" % F, float(e16.mean()))
    record_property("skin32_max_abs_F%d" % F, float(e32.max()))
    assert e16.max() <= max(1.25 * e32.max(), 5e-7) and e16.mean() <= 1.1 * e32.mean()
    assert e16.max() <= VERT_CAP and e32.max() <= VERT_CAP
    # boxes: the exact fp32 min / max of the stored vertices of each 16-vertex unit (the last unit padded with vertex V-1)
    for tag in ("f16", "f32"):
        vs = o["%s_%d_verts" % (tag, F)]
        vp = np.empty((F, 431 * 16, 3), np.float32)
        vp[:, :6890] = vs
        vp[:, 6890:] = vs[:, 6889:6890]
        vp = vp.reshape(F, 431, 16, 3)
        assert np.array_equal(np.concatenate([vp.min(2), vp.max(2)], -1), o["%s_%d_bbox" % (tag, F)]), tag
        # assignment: bit-equal to the brute-force loop (first index on ties) on the closure's own vertices, every frame
        _, i_ref = p3d_ref.knn1_loop(c["markers"].numpy(), vs)
        got = o["%s_%d_nn" % (tag, F)].astype(np.int64)
        present = c["markers"].numpy().any(-1)
        bad = np.argwhere((got != i_ref) & present)
        assert len(bad) == 0, (tag, len(bad), bad[:5].tolist())
    # loss and gradient: x = [trans 3F | z F | betas 10 | pose 207F]
    np.testing.assert_allclose(float(o["f16_%d_loss" % F]), lo, rtol=2e-5)
    blocks = (("trans", slice(0, 3 * F)), ("z", slice(3 * F, 4 * F)), ("betas", slice(4 * F, 4 * F + 10)),
              ("pose", slice(4 * F + 10, None)))
    _check_grad(o["f16_%d_grad" % F], g_ref, blocks, "chamfer_F%d" % F, record_property)


# ------------------------------------------------------------------------------------------------ c. marker closure


def _three_corners(st, vids, seed):
    gen = torch.Generator().manual_seed(seed)
    faces = torch.from_numpy(np.asarray(st.faces).astype(np.int64))
    i3 = torch.zeros(M, 3, dtype=torch.int64)
    b3 = torch.zeros(M, 3)
    for m in range(M):
        hit = (faces == int(vids[m])).any(1).nonzero()
        tri = faces[hit[0, 0]] if len(hit) else torch.tensor([int(vids[m]), (int(vids[m]) + 1) % 6890, (int(vids[m]) + 2) % 6890])
        wt = torch.rand(3, generator=gen) + 0.05
        i3[m], b3[m] = torch.sort(tri)[0], wt / wt.sum()
    return i3.to(torch.int32), b3


@pytest.mark.parametrize("F", [F for F, _ in CASES])
def test_marker_closure_against_float64(smpl, smpl64, st, cases, dev, record_property, F):
    """Gather-LBS marker closure (PT rows, k_bwd_sparse): one-hot and three-corner placements, sigma 0 and 0.05, the
    joint-acceleration term off and on."""
    from uuo_mocap_amd.engine import MarkerProblem

    c = cases[F]
    inp = c["inp"]
    md = c["markers"].to(dev)
    vids = torch.from_numpy(c["vids"]).to(torch.int32)
    i3, b3 = _three_corners(st, c["vids"], F)
    blocks = (("pose", slice(0, 207 * F)), ("betas", slice(207 * F, 207 * F + 10)),
              ("root", slice(207 * F + 10, 216 * F + 10)), ("trans", slice(216 * F + 10, None)))
    for sigma in (0.0, 0.05):
        for accel in (0.0, 1.0):
            cfg = packaged_config("video_mocap")
            cfg["stages"]["marker"]["robust_sigma"] = sigma
            cfg["stages"]["marker"]["losses"]["joint_accel"] = accel
            for assign, bary in ((vids, None), (i3, b3)):
                pm = MarkerProblem(smpl, md, c["o_pose"].to(dev), c["o_betas"].to(dev), assign.to(dev), cfg,
                                   bary=None if bary is None else bary.to(dev))
                x = pm.pack(torch.from_numpy(inp["pose"]).to(dev), torch.from_numpy(inp["betas"]).to(dev),
                            c["root_eval"].to(dev), torch.from_numpy(inp["trans"]).to(dev))
                lm, gm, _ = pm.evaluate(x)
                lo, g_ref = _ref_marker(smpl64, cfg, c["markers"], c["o_pose"], c["o_betas"], x, assign, bary)
                tag = "marker_F%d_%s_s%g_a%g" % (F, "3c" if bary is not None else "1h", sigma, accel)
                np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=tag)
                _check_grad(gm.cpu().numpy(), g_ref, blocks, tag, record_property)


# ------------------------------------------------------------------------------------------------ d. part closure


@pytest.mark.parametrize("F", [F for F, _ in CASES])
def test_part_closure_both_routes_against_float64(smpl, smpl64, st, cases, dev, record_property, F):
    """Part closure on a cached pose: the fused route (k_part_fwd, M <= 16) and the general one (k_skin_cached -> boxes ->
    k_nn_cull, M = 17); two evaluations each, the second on the pose-blend cache of the first."""
    from uuo_mocap_amd.engine import PartProblem

    c = cases[F]
    inp = c["inp"]
    cfg = packaged_config("hmr_part")
    labels = np.argmax(st.lbs_weights, axis=1)
    vidx = torch.from_numpy(np.nonzero(np.isin(labels, [0, 1, 4, 7, 10]))[0]).to(dev)
    blocks = (("z", slice(0, 1)), ("trans", slice(1, 3 * F + 1)), ("betas", slice(3 * F + 1, None)))
    for mk in (16, 17):
        mm = c["markers"][:, :mk].contiguous()
        pp = PartProblem(smpl, mm.to(dev), torch.from_numpy(inp["pose"]).to(dev), c["o_betas"].to(dev),
                         c["root_eval"].to(dev), vidx, cfg)
        x = pp.pack(torch.full((1, 1, 1), 0.2, device=dev), torch.from_numpy(inp["trans"]).to(dev),
                    torch.from_numpy(inp["betas"]).to(dev))
        for k in range(2):
            lp, gp, nnp = pp.evaluate(x)
            lo, g_ref = _ref_part(smpl64, cfg, mm, torch.from_numpy(inp["pose"]), c["o_betas"], c["root_eval"], x, vidx, nnp)
            tag = "part_F%d_M%d_%d" % (F, mk, k)
            np.testing.assert_allclose(lp, lo, rtol=2e-5, err_msg=tag)
            _check_grad(gp.cpu().numpy(), g_ref, blocks, tag, record_property)
            x = x * 0.97 + 0.01


# ------------------------------------------------------------------------------------------------ e. uuo_smpl_backward
@pytest.mark.parametrize("F,frames", [(17, slice(0, 17)), (300, slice(100, 148))])
def test_smpl_backward_against_float64(smpl, smpl64, cases, dev, record_property, F, frames):
    """The dense backward (k_dvp / k_dA / k_dpf and the kinematic tail) with random upstream vertex and joint gradients,
    per-frame betas, against float64 autograd on a block of frames."""
    inp = cases[F]["inp"]
    args = [torch.from_numpy(np.ascontiguousarray(inp[k][frames])) for k in ("pose", "betas_f", "root", "trans")]
    n = args[0].shape[0]
    gen = torch.Generator().manual_seed(F)
    dv = torch.randn(n, 6890, 3, generator=gen)
    dj = torch.randn(n, 45, 3, generator=gen)
    gp, gb, gr, gt = smpl.device_model.smpl_backward(*[a.to(dev) for a in args], dv.to(dev), dj.to(dev))
    with _float64():
        leaves = [a.double().clone().requires_grad_(True) for a in args]
        o = smpl64(*leaves)
        ((o["vertices"] * dv.double()).sum() + (o["joints"] * dj.double()).sum()).backward()
    grad = torch.cat([t.reshape(-1).double().cpu() for t in (gp, gb, gr, gt)]).numpy()
    g_ref = torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()
    a, b, r = 207 * n, 207 * n + 10 * n, 216 * n + 10 * n
    blocks = (("pose", slice(0, a)), ("betas", slice(a, b)), ("root", slice(b, r)), ("trans", slice(r, None)))
    _check_grad(grad, g_ref, blocks, "smpl_backward_F%d" % F, record_property)
