"""The fused closures at marker counts past 50, on every side of the counts at which the code changes path: the marker
groups of the pruned search (k_nn_cull: at most 64 markers a group, G >= 2 from M = 65, at most 8 groups -- 64/65, 128/129,
448/449, 511/512), the switch to the fp32 skinning kernel and the brute-force search (512/513), the part stage's routes
(16/17, 512/513), the 1024-entry chunks of the latent offsets' reduction (3M = 1023, 1026, 1029) and the lock-step launch
with more than one marker group.  Inputs: make_sequence at the marker count of the case, perturbed as everywhere in the suite;
references: float64 autograd (the suite's own restatements) and the CPU brute-force loop on the closure's own vertices.

Bars (the suite's, no new ones): loss rtol 2e-5; gradient < 2e-4 relative as a whole and < 5e-4 per parameter block
(_check_grad); searches, boxes and route comparisons bit for bit.  Observed errors are recorded with record_property."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p3d_ref, stages_ref  # noqa: E402
from foot_lock_ref64 import _cfg as _marker_cfg, _contacts  # noqa: E402
from gpu_support import _check_grad, _inputs, _marker_x, _three_corners, dev, smpl, smpl64  # noqa: E402,F401
from stage_ref64 import _float64, ref_chamfer64, ref_marker64, ref_part64 as _ref_part  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the stage references as this file calls them: the chamfer stage's without rho and with the float64 vertices (as
# test_gpu_model_range.py has it), the marker stage's with foot contacts and the marker count of the case
_ref_chamfer = functools.partial(ref_chamfer64, sigma=0.0, with_vertices=True)


def _ref_marker(smpl64, tables, cfg, markers, o_pose, o_betas, x, assign, bary, contacts, num_markers):
    return ref_marker64(smpl64, tables, cfg, markers, o_pose, o_betas, x, assign, bary, contacts, num_markers=num_markers)

V, NUNITS = 6890, 431
STEP = 1e-3  # between the two evaluations of a case: 1 mm on every translation, 1 mrad on every rotation (a line-search step)

CHAMFER_CASES = [(m, 5) for m in (1, 16, 17, 63, 64, 65, 127, 128, 129, 448, 449, 511, 512, 513, 600)] + [(65, 3)]
SEARCH_ONLY = (64, 1024)  # a full 64-marker group with G = 1 (F G >= 1024 stops the split)
MARKER_CASES = [(m, f) for m in (16, 17, 64, 65, 129, 341, 342, 343, 513) for f in (3, 7)]
PART_CASES = [(m, s) for m in (17, 64, 65, 200, 512, 513) for s in ("body", "leg")]
PART_SUBSETS = {"body": tuple(range(24)), "leg": (0, 1, 4, 7, 10)}
PART_F = 7


def _cull_groups(F, M):
    """Marker groups of the pruned search as uuo_launch_nn_cull documents them: (G, markers per group)."""
    G = (M + 63) // 64
    while G < 8 and F * G < 1024 and (M + G) // (G + 1) >= 8:
        G += 1
    return G, (M + G - 1) // G


def test_group_rule_reaches_the_corners_the_cases_are_named_for():
    assert _cull_groups(3, 65) == (8, 9) and _cull_groups(*SEARCH_ONLY[::-1]) == (1, 64)
    assert _cull_groups(5, 64)[0] > 1 and _cull_groups(5, 512) == (8, 64) and _cull_groups(5, 449) == (8, 57)
    assert _cull_groups(5, 448) == (8, 56) and _cull_groups(5, 129)[1] * (_cull_groups(5, 129)[0] - 1) < 129


def _rodrigues(axis_angle):
    """exp of the skew matrices of `axis_angle` [..., 3] (float64 torch)."""
    th = axis_angle.norm(dim=-1, keepdim=True).clamp_min(1e-30)[..., None]
    k = axis_angle / th[..., 0]
    K = torch.zeros(axis_angle.shape[:-1] + (3, 3), dtype=axis_angle.dtype)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return torch.eye(3, dtype=axis_angle.dtype) + torch.sin(th) * K + (1.0 - torch.cos(th)) * (K @ K)


def _stepped(trans, pose, seed):
    """`trans` moved by STEP metres in a random direction per frame, every rotation of `pose` turned by STEP rad about a
    random axis."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(trans.shape, generator=gen, dtype=torch.float64)
    a = torch.randn(pose.shape[:-2] + (3,), generator=gen, dtype=torch.float64)
    t2 = trans.double() + STEP * d / d.norm(dim=-1, keepdim=True)
    p2 = pose.double() @ _rodrigues(STEP * a / a.norm(dim=-1, keepdim=True))
    return t2.float(), p2.float()


def _run_child(code, timeout=900):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ 1. chamfer closure
_CHAMFER_CHILD = """
import os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from uuo_mocap_amd import _lib
_lib.LIB_PATH = _lib.LIB_DEBUG_PATH  # the kernel-variant knob exists in the debug flavour only
from uuo_mocap_amd import engine
from uuo_mocap_amd.body_model import synthetic_smpl
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.smpl import SmplInference
dev = torch.device('cuda:0')
s = SmplInference(dev, tables=synthetic_smpl(0))
lib = _lib.load_debug()
out = {}
for M, F, tags in %(cases)r:
    d = np.load(os.path.join(%(tmp)r, 'in_%%d_%%d.npz' %% (M, F)))
    g = lambda k: torch.from_numpy(d[k]).to(dev)
    for slot, tag in enumerate(tags):
        engine.set_workspace_slot(slot)  # a workspace of its own: the first search starts without a previous assignment
        os.environ['UUO_SKIN_F16'] = '1' if tag == 'f16' else '0'
        prob = engine.ChamferProblem(s, g('markers'), g('o_pose'), g('o_betas'), g('root'), packaged_config('video_mocap'))
        for k in (0, 1):
            x = prob.pack(g('t%%d' %% k), g('z'), g('b'), g('p%%d' %% k))
            loss, grad, nn = prob.evaluate(x)
            torch.cuda.synchronize()
            verts = np.zeros((F, 6890, 3), np.float32)
            bbox = np.zeros((F, 431, 6), np.float32)
            flags = np.zeros((F, 8), np.int32)
            assert lib.uuo_debug_fit_buffers(prob.fit, verts.ctypes.data, bbox.ctypes.data) == 0
            assert lib.uuo_debug_nn_flags(prob.fit, flags.ctypes.data) == 0
            out.update({'%%s_%%d_%%d_%%d_%%s' %% (tag, M, F, k, n): v for n, v in (
                ('loss', loss), ('grad', grad.cpu().numpy()), ('nn', nn.cpu().numpy()), ('verts', verts), ('bbox', bbox),
                ('flags', flags), ('x', x.cpu().numpy()))})
        del prob
np.savez(os.path.join(%(tmp)r, 'out.npz'), **out)
"""


@pytest.fixture(scope="module")
def chamfer_inputs(tables):
    out = {}
    for M, F in CHAMFER_CASES:
        seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 300 + M + F, M)
        t2, p2 = _stepped(tp, pp, M + F)
        out[(M, F)] = dict(markers=markers, o_pose=o_pose, o_betas=o_betas, root=root, t0=tp, t1=t2, z=zp, b=bp, p0=pp, p1=p2)
    # the search-only case: a 128-frame capture eight times over (the generator's float64 body of 1024 frames alone takes
    # ten seconds), every frame with a perturbation of its own, of _inputs' sizes
    M, F = SEARCH_ONLY
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F // 8, 300 + M + F, M)
    markers, o_pose, root, trans = (t.repeat((8,) + (1,) * (t.dim() - 1)) for t in (markers, o_pose, root, trans))
    gen = torch.Generator().manual_seed(M + F)
    r = lambda *s: torch.randn(*s, generator=gen)
    tp, zp, bp, pp = trans + 0.02 * r(F, 3), 0.3 * r(F, 1, 1), o_betas + 0.3 * r(1, 10), o_pose + 0.05 * r(F, 23, 3, 3)
    t2, p2 = _stepped(tp, pp, M + F)
    out[(M, F)] = dict(markers=markers, o_pose=o_pose, o_betas=o_betas, root=root, t0=tp, t1=t2, z=zp, b=bp, p0=pp, p1=p2)
    return out


@pytest.fixture(scope="module")
def chamfer_runs(chamfer_inputs, tmp_path_factory):
    """One child process on the debug flavour evaluates every case twice -- at x on a fresh workspace (no previous assignment),
    then STEP away from it (pruned from the first evaluation's bounds) -- with UUO_SKIN_F16=1 (k_skin3, the default route) and
    0 (the fp32 k_skin2), and returns loss, gradient, assignment, the stored vertices, the unit boxes and the survivor counts
    of the pruned search."""
    tmp = tmp_path_factory.mktemp("marker_counts_chamfer")
    for (M, F), c in chamfer_inputs.items():
        np.savez(tmp / ("in_%d_%d.npz" % (M, F)), **{k: v.numpy() for k, v in c.items()})
    cases = [(M, F, ("f16", "f32")) for M, F in CHAMFER_CASES] + [SEARCH_ONLY + (("f16",),)]
    _run_child(_CHAMFER_CHILD % dict(root=ROOT, tmp=str(tmp), cases=cases))
    return np.load(tmp / "out.npz")


def _check_search(o, key, markers, tag):
    """The assignment against the CPU brute-force loop (first index on ties) on the closure's own stored vertices: every frame,
    every marker whose row is not all zero."""
    _, i_ref = p3d_ref.knn1_loop(markers, o[key + "_verts"])
    got = o[key + "_nn"].astype(np.int64)
    bad = np.argwhere((got != i_ref) & markers.any(-1))
    assert len(bad) == 0, (tag, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("M,F", CHAMFER_CASES)
def test_chamfer_closure_across_marker_counts(smpl64, chamfer_inputs, chamfer_runs, record_property, M, F):
    """k_skin3 / k_skin2 -> unit boxes -> k_nn_cull (M <= 512) or k_skin2 -> k_nn (M > 512), then k_bwd_sparse and finalize:
    assignment, boxes, loss, gradient and the route taken, at both evaluations of both skinning kernels."""
    c, o = chamfer_inputs[(M, F)], chamfer_runs
    cfg = packaged_config("video_mocap")
    markers = c["markers"].numpy()
    G, mper = _cull_groups(F, M)
    blocks = (("trans", slice(0, 3 * F)), ("z", slice(3 * F, 4 * F)), ("betas", slice(4 * F, 4 * F + 10)),
              ("pose", slice(4 * F + 10, None)))
    refs = {}
    for k in (0, 1):
        for tag in ("f16", "f32"):
            key = "%s_%d_%d_%d" % (tag, M, F, k)
            name = "chamfer_M%d_F%d_%s_%d" % (M, F, tag, k)
            _check_search(o, key, markers, name)
            flags = o[key + "_flags"]
            if M <= 512:
                vs = o[key + "_verts"]   # boxes: the exact fp32 min / max of each 16-vertex unit (the last padded with V - 1)
                vp = np.empty((F, NUNITS * 16, 3), np.float32)
                vp[:, :V] = vs
                vp[:, V:] = vs[:, V - 1:V]
                vp = vp.reshape(F, NUNITS, 16, 3)
                assert np.array_equal(np.concatenate([vp.min(2), vp.max(2)], -1), o[key + "_bbox"]), name
                assert (flags[:, :G] != 0).all() and not flags[:, G:].any(), (name, G, flags.tolist())
                pruned = flags[:, :G] > 0   # (a negative count: the block's survivor list overflowed, every pair enumerated)
                record_property("pruned_share_%s" % name, float(pruned.mean()))
                print("%s: %d groups of <= %d markers, pruned blocks %d of %d, most survivors per group %s"
                      % (name, G, mper, pruned.sum(), pruned.size, np.abs(flags[:, :G]).max(0).tolist()))
                if k == 1:   # from the first evaluation's bounds the lists must hold, in some block of every marker group
                    assert pruned.any(0).all(), (name, flags.tolist())
            else:
                assert not flags.any(), (name, flags.tolist())   # a fresh workspace's zeros: k_nn_cull never ran
            # loss and gradient against float64 on the closure's assignment (one reference per distinct assignment)
            rk = (k, o[key + "_nn"].tobytes())
            if rk not in refs:
                refs[rk] = _ref_chamfer(smpl64, cfg, c["markers"], c["o_pose"], c["o_betas"], c["root"], o[key + "_x"],
                                        o[key + "_nn"].astype(np.int64))[:2]
            lo, g_ref = refs[rk]
            loss = float(o[key + "_loss"])
            record_property("loss_rel_%s" % name, abs(loss - lo) / abs(lo))
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
            _check_grad(o[key + "_grad"], g_ref, blocks, name, record_property)
        if M > 512:   # both flavours skin with k_skin2 and search with k_nn: the same launches
            a, b = "f16_%d_%d_%d" % (M, F, k), "f32_%d_%d_%d" % (M, F, k)
            for n in ("loss", "grad", "nn", "verts"):
                assert np.array_equal(o[a + "_" + n], o[b + "_" + n]), (M, F, k, n)


def test_pruned_search_on_a_full_group(chamfer_inputs, chamfer_runs):
    """M = 64 at F = 1024: one group of 64 markers per frame (every slot of the 64-wide LDS arrays in use)."""
    M, F = SEARCH_ONLY
    assert _cull_groups(F, M) == (1, 64)
    markers = chamfer_inputs[SEARCH_ONLY]["markers"].numpy()
    for k in (0, 1):
        key = "f16_%d_%d_%d" % (M, F, k)
        _check_search(chamfer_runs, key, markers, key)
        flags = chamfer_runs[key + "_flags"]
        assert (flags[:, 0] != 0).all() and not flags[:, 1:].any()
    assert (flags[:, 0] > 0).any()


# ------------------------------------------------------------------------------------------------ 2. marker closures
def _packing_solves(prob, x0, dev, tag):
    """solve(max_iter=3) on the compact and on the full packing (UUO_NO_COMPACT=1, debug flavour) as in
    test_compact_and_full_packings_agree_and_solves_are_deterministic: the driver's decisions rest on g.d, sum|g|, g.g and
    max|g| over the whole vector, the offsets' entries included."""
    from uuo_mocap_amd import _lib
    from uuo_mocap_amd._lib import UuoLbfgsOptions, UuoLbfgsStats
    from uuo_mocap_amd.engine import _ptr, current_stream

    dbg = _lib.load_debug()
    M = prob.M

    def solve(no_compact):
        x = x0.clone()
        losses = []
        cb = _lib.EVAL_CALLBACK(lambda user, i, loss, d_x_eval: losses.append(loss))
        opt = UuoLbfgsOptions(3, 100, 1.0, 1e-7, 1e-9, 0, 0)
        st = UuoLbfgsStats()
        os.environ["UUO_NO_COMPACT"] = "1" if no_compact else "0"
        try:
            prob._arm()
            rc = dbg.uuo_lbfgs_solve(prob.fit, current_stream(dev), ctypes.byref(prob.problem), _ptr(x), ctypes.byref(opt),
                                     ctypes.byref(st), ctypes.cast(cb, ctypes.c_void_p), None)
        finally:
            os.environ.pop("UUO_NO_COMPACT", None)
        assert rc == 0, dbg.uuo_last_error()
        torch.cuda.synchronize()
        return x, losses, (st.n_iter, st.n_eval, st.stop_reason)

    xc, lc, sc = solve(False)
    xf, lf, sf = solve(True)
    head = min(len(lc), len(lf), 40)
    assert head >= 2, (tag, lc, lf)
    np.testing.assert_allclose(lc[:head], lf[:head], rtol=1e-6, err_msg=tag)
    assert abs(sc[0] - sf[0]) <= 2 and abs(sc[1] - sf[1]) <= 3, (tag, sc, sf)
    assert float((xc - xf).abs().max()) < 1e-3, tag
    assert not torch.equal(xc[-3 * M:], x0[-3 * M:]), tag
    xc2, lc2, sc2 = solve(False)
    assert torch.equal(xc, xc2) and lc == lc2 and sc == sc2, tag


@pytest.mark.parametrize("M,F", MARKER_CASES)
def test_marker_closures_across_marker_counts(smpl, smpl64, tables, dev, record_property, M, F):
    """k_bwd_sparse / k_bary_fwd + k_bwd_items in rounds of 16 items (3M items with three corners), finalize_body<OFFS> in
    chunks of 1024 of the 3M offset entries (M = 341, 342, 343, 513: a tail chunk of none, 2, 5 and 515 entries): one-hot and
    three-corner placements; plain, robust, latent offsets alone and with the two temporal terms."""
    from uuo_mocap_amd.engine import MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 500 + M + F, M)
    contacts = _contacts(F, F)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, M)
    n0 = 219 * F + 10
    blocks = (("pose", slice(0, 207 * F)), ("betas", slice(207 * F, 207 * F + 10)),
              ("root", slice(207 * F + 10, 216 * F + 10)), ("trans", slice(216 * F + 10, n0)))
    configs = (("plain", _marker_cfg(0.0, 0.0)), ("robust", _marker_cfg(0.0, 0.0, sigma=0.05)),
               ("offsets", _marker_cfg(0.0, 0.0, offs=True)), ("offsets_accel_lock", _marker_cfg(100.0, 10.0, accel=True, offs=True)))
    for cname, cfg in configs:
        for assign, bary in ((vids, None), (i3, b3)):
            pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), assign.to(dev), cfg,
                               bary=None if bary is None else bary.to(dev), foot_contacts=contacts)
            offs = cname.startswith("offsets")
            assert pm.has_offsets == offs and pm.n == n0 + (3 * M if offs else 0)
            assert (pm.foot_lock > 0.0 and pm.joint_accel > 0.0) == (cname == "offsets_accel_lock")
            xm = _marker_x(pm, pp, bp, rp, tp, dev, F, M)
            lm, gm, _ = pm.evaluate(xm, want_nn=False)
            lm2, gm2, _ = pm.evaluate(xm, want_nn=False)
            name = "marker_M%d_F%d_%s_%s" % (M, F, "3c" if bary is not None else "1h", cname)
            assert lm == lm2 and torch.equal(gm, gm2), name
            lo, g_ref = _ref_marker(smpl64, tables, cfg, markers, o_pose, o_betas, xm, assign, bary, contacts, M)
            record_property("loss_rel_%s" % name, abs(lm - lo) / abs(lo))
            np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=name)
            _check_grad(gm.cpu().numpy(), g_ref, blocks + ((("offsets", slice(n0, None)),) if offs else ()), name,
                        record_property)
            if cname == "offsets_accel_lock" and M in (341, 342, 343):
                x0 = pm.pack(o_pose.to(dev), o_betas.to(dev), root.to(dev), trans.to(dev))   # (third rows on their targets)
                x0[n0:] = pm.offsets_start(x0).reshape(-1)
                _packing_solves(pm, x0, dev, name)


# ------------------------------------------------------------------------------------------------ 3. part closure
_PART_CHILD = """
import os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from uuo_mocap_amd import _lib
_lib.LIB_PATH = _lib.LIB_DEBUG_PATH  # the search knob exists in the debug flavour only
from uuo_mocap_amd import engine
from uuo_mocap_amd.body_model import synthetic_smpl
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.smpl import SmplInference
dev = torch.device('cuda:0')
s = SmplInference(dev, tables=synthetic_smpl(0))
lib = _lib.load_debug()
out = {}
F = %(frames)d
for case, (M, sub) in enumerate(%(cases)r):
    d = np.load(os.path.join(%(tmp)r, 'in_%%d_%%s.npz' %% (M, sub)))
    g = lambda k: torch.from_numpy(d[k]).to(dev)
    for j, brute in enumerate(('0', '1')):
        # a workspace of its own (both subsets of a marker count have one shape): the first search starts without a
        # previous assignment, and the survivor counts tell whether the pruned search ran
        engine.set_workspace_slot(2 * case + j)
        os.environ['UUO_PART_BRUTE'] = brute
        prob = engine.PartProblem(s, g('markers'), g('pose'), g('o_betas'), g('root'), g('vidx'), packaged_config('hmr_part'))
        for k in (0, 1):
            loss, grad, nn = prob.evaluate(g('x%%d' %% k))
            torch.cuda.synchronize()
            flags = np.zeros((F, 8), np.int32)
            assert lib.uuo_debug_nn_flags(prob.fit, flags.ctypes.data) == 0
            out.update({'%%s_%%d_%%s_%%d_%%s' %% (brute, M, sub, k, n): v for n, v in (
                ('loss', loss), ('grad', grad.cpu().numpy()), ('nn', nn.cpu().numpy()), ('flags', flags))})
        del prob
np.savez(os.path.join(%(tmp)r, 'out.npz'), **out)
"""


@pytest.fixture(scope="module")
def part_inputs(tables):
    labels = np.argmax(tables.lbs_weights, axis=1)
    out = {}
    for M, sub in PART_CASES:
        seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, PART_F, 700 + M, M)
        vidx = torch.from_numpy(np.nonzero(np.isin(labels, PART_SUBSETS[sub]))[0])
        x0 = torch.cat([torch.full((1,), 0.2), tp.reshape(-1), bp.reshape(-1)])
        gen = torch.Generator().manual_seed(M)
        x1 = x0 + 2.0 * STEP * torch.randn(x0.shape, generator=gen)
        out[(M, sub)] = dict(markers=markers, pose=o_pose, o_betas=o_betas, root=root, vidx=vidx, x0=x0, x1=x1)
    return out


@pytest.fixture(scope="module")
def part_runs(part_inputs, tmp_path_factory):
    """One child process on the debug flavour: every case at two points, on the default route and with UUO_PART_BRUTE=1."""
    tmp = tmp_path_factory.mktemp("marker_counts_part")
    for (M, sub), c in part_inputs.items():
        np.savez(tmp / ("in_%d_%s.npz" % (M, sub)), **{k: v.numpy() for k, v in c.items()})
    _run_child(_PART_CHILD % dict(root=ROOT, tmp=str(tmp), cases=PART_CASES, frames=PART_F))
    return np.load(tmp / "out.npz")


@pytest.mark.parametrize("M,sub", PART_CASES)
def test_part_closure_across_marker_counts(smpl64, part_inputs, part_runs, record_property, M, sub):
    """Part stage on a cached pose: k_skin_cached + boxes + k_nn_cull on the subset's compact cloud up to M = 512, k_skin_cached
    + k_nn beyond; against the brute-force route bit for bit and against float64."""
    c, o = part_inputs[(M, sub)], part_runs
    cfg = packaged_config("hmr_part")
    F = PART_F
    G = _cull_groups(F, M)[0]
    blocks = (("z", slice(0, 1)), ("trans", slice(1, 3 * F + 1)), ("betas", slice(3 * F + 1, None)))
    for k in (0, 1):
        a, b = "0_%d_%s_%d" % (M, sub, k), "1_%d_%s_%d" % (M, sub, k)
        name = "part_M%d_%s_%d" % (M, sub, k)
        for n in ("loss", "grad", "nn"):
            assert np.array_equal(o[a + "_" + n], o[b + "_" + n]), (name, n)
        assert o[a + "_nn"].min() >= 0 and o[a + "_nn"].max() < len(c["vidx"])
        assert not o[b + "_flags"].any(), name   # (the brute-force route leaves its fresh workspace's zeros)
        if M <= 512:
            assert (o[a + "_flags"][:, :G] != 0).all() and not o[a + "_flags"][:, G:].any(), (name, o[a + "_flags"].tolist())
        else:
            assert not o[a + "_flags"].any(), name
        lo, g_ref = _ref_part(smpl64, cfg, c["markers"], c["pose"], c["o_betas"], c["root"], c["x%d" % k], c["vidx"],
                              torch.from_numpy(o[a + "_nn"]))
        loss = float(o[a + "_loss"])
        record_property("loss_rel_%s" % name, abs(loss - lo) / abs(lo))
        np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
        _check_grad(o[a + "_grad"], g_ref, blocks, name, record_property)


# ------------------------------------------------------------------------------------------------ 4. soft chamfer closure
@pytest.mark.parametrize("M", [65, 512, 513])
def test_soft_chamfer_closure_across_marker_counts(smpl, smpl64, tables, dev, record_property, M):
    """The soft-assignment chamfer closure (all 6 890 vertices per marker, dense backward) on both sides of the switch between
    the box-assisted soft-min (M <= 512) and the one without boxes: test_fused_soft_chamfer_closure_against_float64's
    objective, 10 (-tau logsumexp(-d^2 / tau)) masked and normalised plus the priors, in float64 autograd."""
    from uuo_mocap_amd.engine import ChamferProblem

    F, tau = 5, 1e-3
    cfg = copy.deepcopy(packaged_config("video_mocap"))
    lw = cfg["stages"]["chamfer"]["losses"]
    lw["soft_chamfer"] = 10.0
    cfg["stages"]["chamfer"]["soft_tau"] = tau
    del lw["full_chamfer"]
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 900 + M, M)
    prob = ChamferProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    assert prob.problem.w_soft == 10.0
    x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    loss, grad, nn = prob.evaluate(x)
    loss2, grad2, _ = prob.evaluate(x)
    assert loss2 == loss and torch.equal(grad, grad2), "the fused soft closure must be bit-reproducible"
    with _float64():
        leaves = [t.double().clone().requires_grad_(True) for t in (tp, zp, bp, pp)]
        z_root = stages_ref.compute_root_orient_z(leaves[1]) @ root.double()
        vs = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(leaves[3]), leaves[2],
                                           stages_ref.normalize_rot(z_root), leaves[0])["vertices"]
        mask = stages_ref.get_marker_mask(markers.double()).double()
        ref = 0.0
        for f in range(F):   # a frame at a time: [M, V, 3] float64 differences
            d2 = ((markers[f].double()[:, None] - vs[f][None]) ** 2).sum(-1)
            ref = ref + (10.0 * (-tau * torch.logsumexp(-d2 / tau, dim=-1)) * mask[f]).sum() / mask.sum()
        ref = ref + lw["reg_pose_body"] * ((leaves[3] - o_pose.double()) ** 2).mean() + \
            lw["reg_betas"] * ((leaves[2] - o_betas.double()) ** 2).mean()
        ref.backward()
    g_ref = torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()
    name = "soft_chamfer_M%d_F%d" % (M, F)
    lo = float(ref.detach())
    record_property("loss_rel_%s" % name, abs(loss - lo) / abs(lo))
    np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
    blocks = (("trans", slice(0, 3 * F)), ("z", slice(3 * F, 4 * F)), ("betas", slice(4 * F, 4 * F + 10)),
              ("pose", slice(4 * F + 10, None)))
    _check_grad(grad.cpu().numpy(), g_ref, blocks, name, record_property)
    hard = ChamferProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), packaged_config("video_mocap"))
    _, _, nn_hard = hard.evaluate(x)
    assert torch.equal(nn, nn_hard), "the assignment it reports is the hard closure's"


# ------------------------------------------------------------------------------------------------ 5. routes
def test_lockstep_batch_with_marker_groups_is_bit_identical_to_solving_one_by_one(smpl, tables, dev):
    """Four yaw hypotheses of the chamfer stage at M = 70, F = 12 (G = 8 groups of 9 markers: k_nn_cull_b takes its grid's y
    extent from the recorded launch): uuo_batch_solve must end where uuo_lbfgs_solve takes each problem alone."""
    from uuo_mocap_amd.engine import ChamferProblem, solve_batch
    from uuo_mocap_amd.transforms import compute_root_orient_z

    F, M = 12, 70
    assert _cull_groups(F, M)[0] >= 2
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 31, M)
    cfg = packaged_config("video_mocap")
    md, o_pose, o_betas, root, trans = (t.to(dev) for t in (markers, o_pose, o_betas, root, trans))

    def problems():
        return [ChamferProblem(smpl, md, o_pose, o_betas,
                               (compute_root_orient_z(torch.full((F, 1, 1), k * np.pi / 2, device=dev)) @ root).contiguous(), cfg)
                for k in range(4)]

    probs_a, probs_b = problems(), problems()
    xs_a = [p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose) for p in probs_a]
    xs_b = [x.clone() for x in xs_a]
    alone = [p.solve(x, max_iter=25, lr=0.1) for p, x in zip(probs_a, xs_a)]
    together = solve_batch(probs_b, xs_b, max_iter=25, lr=0.1)
    for i, (sa, sb, xa, xb) in enumerate(zip(alone, together, xs_a, xs_b)):
        assert (sa["n_iter"], sa["n_eval"], sa["stop_reason"]) == (sb["n_iter"], sb["n_eval"], sb["stop_reason"]), (i, sa, sb)
        assert sa["first_loss"] == sb["first_loss"] and sa["final_loss"] == sb["final_loss"], (i, sa, sb)
        assert sa["final_loss"] < sa["first_loss"], (i, sa)
        assert torch.equal(xa, xb), "problem %d: iterates differ" % i


def test_whole_fit_at_70_markers(smpl, tables, dev):
    """multimodal_video_mocap with the packaged video_mocap config at M = 70, F = 12: finite, every solve of the config's
    stages (part, chamfer, marker) reduces its loss, the closing repeat of the marker stage -- which starts from that stage's
    end -- does not raise it, and a second run gives the same result bit for bit."""
    from uuo_mocap_amd.multimodal import last_run_stats, multimodal_video_mocap

    seq = make_sequence(tables, seed=17, num_frames=12, num_markers=70)
    outs = []
    for _ in range(2):
        outs.append(multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(seq.markers.get_points().copy(), 30.0),
                                           dev, packaged_config("video_mocap"), offset=0, print_options=[], save_stages=False,
                                           smpl_inference=smpl))
        st = copy.deepcopy(dict(last_run_stats()))
        for stage in ("part", "chamfer", "marker", "marker_final"):
            assert len(st[stage]) > 0, stage
            for s_ in st[stage]:
                assert np.isfinite(s_["final_loss"]) and s_["final_loss"] <= s_["first_loss"], (stage, s_)
                assert stage == "marker_final" or s_["final_loss"] < s_["first_loss"], (stage, s_)
    for key in ("pose_body", "betas", "root_orient", "trans"):
        a, b = torch.as_tensor(outs[0][key]), torch.as_tensor(outs[1][key])
        assert torch.isfinite(a).all(), key
        assert torch.equal(a, b), key


@pytest.mark.parametrize("M", [65, 130])
def test_marker_placement_bit_exact_past_64_markers(smpl, oracle_smpl, dev, M):
    """uuo_assign_mean_argmin against the numpy-semantics C restatement (test_marker_placement_bit_exact's check)."""
    F = 12
    seq = make_sequence(smpl.tables, seed=6, num_frames=F, num_markers=M)
    gt = seq.gt
    t = lambda a: torch.from_numpy(np.asarray(a)).clone()
    verts = oracle_smpl(t(gt["rot"][:, 1:]), t(gt["betas"]).repeat(F, 1), t(gt["rot"][:, :1]), t(gt["trans"]))["vertices"].numpy()
    markers = seq.markers.get_points().astype(np.float32)
    valid = np.ones(F, dtype=np.uint8)
    valid[[2, 7]] = 0
    lib = p3d_ref._load_knn_c()
    out_idx = np.zeros(M, dtype=np.int64)
    lib.assign_mean_argmin_cpu.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 2
    lib.assign_mean_argmin_cpu(verts.ctypes.data, markers.ctypes.data, valid.ctypes.data, F, M, V, out_idx.ctypes.data, None)
    idx = smpl.device_model.assign_mean_argmin(t(verts).to(dev), t(markers).to(dev), t(valid.astype(bool)).to(dev))
    np.testing.assert_array_equal(idx.cpu().numpy(), out_idx)


@pytest.mark.parametrize("M", [65, 130])
def test_rigidity_matrix_bit_equal_past_64_markers(dev, M):
    """uuo_rigid_distance_std against the per-pair np.std(np.linalg.norm(...)) loop
    (test_rigidity_matrix_kernel_is_bit_equal_to_numpy's check), with a stretch of missing markers."""
    from uuo_mocap_amd import markers_utils as MU

    rng = np.random.default_rng(M)
    for F in (20, 129):
        p = (rng.standard_normal((F, M, 3)) * 0.4).astype(np.float32)
        p[3:11, M - 1] = 0.0  # missing markers are exact zeros
        loop = np.zeros((M, M))
        for i in range(M):
            for j in range(M):
                loop[i, j] = np.std(np.linalg.norm(p[:, i] - p[:, j], axis=-1))
        got = MU.rigid_distance_matrix(torch.from_numpy(p).to(dev))
        assert got.dtype == np.float64 and np.array_equal(got, loop), (F, M, np.abs(got - loop).max())
        assert np.array_equal(MU.rigid_distance_matrix(p, device=dev), loop)
