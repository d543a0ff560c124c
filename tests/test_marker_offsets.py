"""EXTENSION: latent per-marker offsets of the marker stage (stages.marker.losses.latent_offsets, uuo_problem_t.w_offsets) --
config validation, the routes that refuse the term, the C ABI layout and parameter count, the compact index map, a float64
restatement of the loss and gradient against central differences, and the stand-off capture of the synthetic generator.  No GPU
needed (tests/test_gpu_marker_offsets.py holds the closures)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0 = 0.0095


def _cfg(**marker_losses):
    from uuo_mocap_amd.config import packaged_config

    cfg = packaged_config("video_mocap")
    cfg["stages"]["marker"]["losses"].update(marker_losses)
    return cfg


# ------------------------------------------------------------------------------------------------ config
def test_key_is_read_and_validated():
    from uuo_mocap_amd.engine import stage_latent_offsets

    assert stage_latent_offsets(_cfg()) == 0.0                                  # absent: off
    assert stage_latent_offsets(_cfg(latent_offsets=0)) == 0.0
    assert stage_latent_offsets(_cfg(latent_offsets=None)) == 0.0
    assert stage_latent_offsets(_cfg(latent_offsets=0.5)) == pytest.approx(0.5)
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="latent_offsets"):
            stage_latent_offsets(_cfg(latent_offsets=bad))


def test_shipped_config_differs_from_its_parent_by_the_key_only():
    from uuo_mocap_amd.config import packaged_config

    plain, offs = packaged_config("video_mocap"), packaged_config("video_mocap_offsets")
    w = offs["stages"]["marker"]["losses"].pop("latent_offsets")
    assert w > 0.0
    for k in ("name", "parent"):
        offs.pop(k, None)
        plain.pop(k, None)
    assert offs == plain


def test_other_stages_and_routes_refuse_the_term():
    import torch

    from uuo_mocap_amd import optimization
    from uuo_mocap_amd._lib import UuoProblem
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch

    cfg = _cfg(latent_offsets=1.0)
    cfg["stages"]["chamfer"]["losses"]["latent_offsets"] = 1.0
    cfg["stages"]["part"]["losses"]["latent_offsets"] = 1.0
    with pytest.raises(NotImplementedError, match="latent_offsets"):
        ChamferProblem(None, None, None, None, None, cfg)
    with pytest.raises(NotImplementedError, match="latent_offsets"):
        PartProblem(None, None, None, None, None, None, cfg)
    cfg = _cfg(latent_offsets=1.0)
    assert not optimization.lockstep_supported(cfg, "marker")
    assert optimization.lockstep_supported(_cfg(latent_offsets=0.0), "marker")
    assert optimization.lockstep_supported(cfg, "chamfer")
    t = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="latent_offsets.*composed"):
        optimization._optim_markers_general(t, t, t, t, t, t, t, t, None, cfg, False)
    with pytest.raises(NotImplementedError, match="latent_offsets.*sharding"):
        optimization._optim_markers_frame_sharded(None, t, t, t, t, t, t, t, t, None, cfg, None)
    p = UuoProblem()
    p.w_offsets = 1.0
    fake = types.SimpleNamespace(joint_accel=0.0, problem=p, model=None)
    with pytest.raises(NotImplementedError, match="latent"):
        solve_batch([fake], [t], max_iter=1)
    # use_sdf keeps its own refusal and message
    cfg["stages"]["marker"]["use_sdf"] = True
    assert not optimization.lockstep_supported(cfg, "marker")


# ------------------------------------------------------------------------------------------------ C ABI
def test_problem_struct_ends_with_w_offsets_and_matches_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    header = open(os.path.join(ROOT, "include", "uuo_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header.split("enum { UUO_STAGE_CHAMFER")[1].split("} uuo_problem_t;")[0], flags=re.S)
    fields = re.findall(r"\b(\w+);", body)
    assert fields[-2:] == ["robust_sigma", "w_offsets"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uuo_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(uuo_problem_t), offsetof(uuo_problem_t, robust_sigma), '
                   'offsetof(uuo_problem_t, w_offsets)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_rs, off_w = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(_lib.UuoProblem)
    assert off_rs == _lib.UuoProblem.robust_sigma.offset
    assert off_w == _lib.UuoProblem.w_offsets.offset and off_w + _lib.UuoProblem.w_offsets.size <= size
    assert off_w > max(f.offset for f in (getattr(_lib.UuoProblem, n) for n, _ in _lib.UuoProblem._fields_))
    p = _lib.UuoProblem()
    assert p.w_offsets == 0.0            # a fresh structure is the term off
    p.w_offsets, p.robust_sigma = 2.5, 0.05
    assert p.w_offsets == 2.5 and p.robust_sigma == pytest.approx(0.05)
    q = _lib.UuoProblem()
    ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(p))   # (how solve_batch copies problems)
    assert q.w_offsets == 2.5
    assert _lib.ABI_VERSION == 3


def test_num_params_counts_the_offsets_of_the_marker_stage_only():
    from uuo_mocap_amd import _lib

    lib = _lib.load()
    for stage, per_frame, const in ((_lib.UUO_STAGE_CHAMFER, 211, 10), (_lib.UUO_STAGE_MARKER, 219, 10),
                                    (_lib.UUO_STAGE_PART, 3, 11)):
        for F in (1, 30, 300):
            for M in (1, 50):
                p = _lib.UuoProblem()
                p.stage, p.F, p.M = stage, F, M
                assert lib.uuo_problem_num_params(ctypes.byref(p)) == per_frame * F + const
                p.w_offsets = 1.0
                extra = 3 * M if stage == _lib.UUO_STAGE_MARKER else 0
                assert lib.uuo_problem_num_params(ctypes.byref(p)) == per_frame * F + const + extra


def test_compact_index_map_reaches_every_coordinate_with_the_offsets_once():
    """Compact packing: every coordinate of [pose 207F | betas 10 | root 9F | trans 3F | offsets 3M] except entries 6..8 of each
    rotation, in order, each exactly once; the full packing is the identity over all 219F + 10 + 3M."""
    from uuo_mocap_amd import _lib

    dbg = _lib.load_debug()
    keep9 = np.arange(9) < 6
    for F in (1, 7, 300):
        for M in (1, 50, 400):
            p = _lib.UuoProblem()
            p.stage, p.F, p.M, p.w_offsets = _lib.UUO_STAGE_MARKER, F, M, 1.0
            n_full = 219 * F + 10 + 3 * M
            keep = np.concatenate([np.tile(keep9, 23 * F), np.ones(10, bool), np.tile(keep9, F), np.ones(3 * F + 3 * M, bool)])
            assert keep.size == n_full
            out = np.full(n_full, -1, np.int32)
            n = dbg.uuo_debug_problem_index_map(ctypes.byref(p), 1, out.ctypes.data)
            assert n == int(keep.sum()) == 147 * F + 10 + 3 * M
            assert np.array_equal(out[:n], np.nonzero(keep)[0])
            assert np.unique(out[:n]).size == n
            assert np.array_equal(out[n - 3 * M:n], np.arange(219 * F + 10, n_full))
            n = dbg.uuo_debug_problem_index_map(ctypes.byref(p), 0, out.ctypes.data)
            assert n == n_full and np.array_equal(out, np.arange(n_full))
            p.w_offsets = 0.0   # the term off: the map of the stage without it
            ref = np.full(219 * F + 10, -1, np.int32)
            n0 = dbg.uuo_debug_index_map(_lib.UUO_STAGE_MARKER, F, 1, ref.ctypes.data)
            n = dbg.uuo_debug_problem_index_map(ctypes.byref(p), 1, out.ctypes.data)
            assert n == n0 and np.array_equal(out[:n], ref[:n0])


# ------------------------------------------------------------------------------------------------ float64 restatement
def _model64(F, seed):
    from uuo_mocap_amd.body_model import synthetic_smpl
    from uuo_mocap_amd.synthetic import lbs_f64, make_sequence

    tables = synthetic_smpl(0)
    seq = make_sequence(tables, seed=seed, num_frames=F, num_markers=12)
    verts, _, T_R = lbs_f64(tables, seq.gt["rot"].astype(np.float64), seq.gt["betas"].astype(np.float64),
                            seq.gt["trans"].astype(np.float64))
    vids = np.asarray(seq.gt["marker_vids"])
    x = np.asarray(seq.markers.get_points(), np.float64).copy()
    x[2, 3] = 0.0   # one missing observation
    return x, verts[:, vids], T_R[:, vids]


def _loss_grad(x, v, T_R, o, w_data, w, sigma=0.0):
    """loss = w_data/(F M) sum mask rho(|x - (v + T_R o)|^2) + w/M sum (|o| - d0)^2 and its gradient in o (float64)."""
    F, M = x.shape[:2]
    mask = (np.abs(x).sum(-1) != 0).astype(np.float64)
    r = x - (v + np.einsum("fmab,mb->fma", T_R, o))
    s = (r * r).sum(-1)
    q = sigma ** 2 / (sigma ** 2 + s) if sigma else np.ones_like(s)
    ln = np.linalg.norm(o, axis=1)
    loss = w_data / (F * M) * (mask * s * q).sum() + w / M * ((ln - D0) ** 2).sum()
    g = -(2.0 * w_data / (F * M)) * np.einsum("fm,fmba,fmb->ma", mask * q * q, T_R, r)
    g += np.where(ln[:, None] > 0, (2.0 * w / M) * (ln - D0)[:, None] * o / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    return loss, g


@pytest.mark.parametrize("sigma", [0.0, 0.01])
def test_float64_loss_and_gradient_match_central_differences(sigma):
    x, v, T_R = _model64(6, 4)
    M = x.shape[1]
    rng = np.random.default_rng(0)
    o = rng.normal(size=(M, 3))
    o *= (D0 * rng.uniform(0.6, 1.5, size=(M, 1))) / np.linalg.norm(o, axis=1, keepdims=True)
    _, g = _loss_grad(x, v, T_R, o, 1.0, 3.0, sigma)
    h = 1e-7
    num = np.zeros_like(o)
    for m in range(M):
        for c in range(3):
            op, om = o.copy(), o.copy()
            op[m, c] += h
            om[m, c] -= h
            num[m, c] = (_loss_grad(x, v, T_R, op, 1.0, 3.0, sigma)[0] - _loss_grad(x, v, T_R, om, 1.0, 3.0, sigma)[0]) / (2 * h)
    np.testing.assert_allclose(g, num, rtol=1e-5, atol=1e-9)
    # the prior alone: zero gradient at o = 0, loss d0^2 per marker
    l0, g0 = _loss_grad(x * 0.0, v, T_R, np.zeros((M, 3)), 1.0, 3.0)
    assert not g0.any() and l0 == pytest.approx(3.0 * D0 ** 2)


def test_start_value_recovers_the_generator_offsets_at_the_true_pose():
    """At the true pose the plain data gradient at o = 0 is -(2/(F M)) sum mask T_R^T (x - v): the masked mean residual in the
    marker's frame, i.e. (up to the 1 mm noise) the generator's own 9.5 mm outward offset, whose direction the start value
    takes."""
    from uuo_mocap_amd.body_model import synthetic_smpl
    from uuo_mocap_amd.synthetic import make_sequence

    x, v, T_R = _model64(40, 2)
    _, g = _loss_grad(x, v, T_R, np.zeros((x.shape[1], 3)), 1.0, 0.0)
    o0 = D0 * -g / np.linalg.norm(g, axis=1, keepdims=True)
    true = make_sequence(synthetic_smpl(0), seed=2, num_frames=40, num_markers=12).gt["marker_offsets"]
    assert np.abs(o0 - true).max() < 1.5e-3


# ------------------------------------------------------------------------------------------------ synthetic stand-off capture
def test_standoff_capture():
    from uuo_mocap_amd.body_model import synthetic_smpl
    from uuo_mocap_amd.synthetic import make_sequence

    tables = synthetic_smpl(0)
    plain = make_sequence(tables, seed=1, num_frames=20, num_markers=30)
    same = make_sequence(tables, seed=1, num_frames=20, num_markers=30, standoff_tilt_deg=0.0, standoff_mm=(9.5, 9.5))
    off = make_sequence(tables, seed=1, num_frames=20, num_markers=30, standoff_tilt_deg=30.0, standoff_mm=(8.0, 14.0))
    assert np.array_equal(plain.markers.get_points(), same.markers.get_points())
    for k in plain.gt:
        assert np.array_equal(plain.gt[k], same.gt[k]), k
        if k != "marker_offsets":
            assert np.array_equal(plain.gt[k], off.gt[k]), k
    assert np.array_equal(plain.img_smpl.pose_body.numpy(), off.img_smpl.pose_body.numpy())
    o_plain, o_off = plain.gt["marker_offsets"].astype(np.float64), off.gt["marker_offsets"].astype(np.float64)
    assert o_plain.shape == o_off.shape == (30, 3)
    np.testing.assert_allclose(np.linalg.norm(o_plain, axis=1), D0, rtol=1e-6)
    ln = np.linalg.norm(o_off, axis=1)
    assert ln.min() >= 0.008 - 1e-7 and ln.max() <= 0.014 + 1e-7 and ln.max() - ln.min() > 0.003
    cosang = np.sum(o_off * o_plain, axis=1) / (ln * np.linalg.norm(o_plain, axis=1))
    ang = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
    assert ang.max() <= 30.0 + 1e-3 and ang.max() > 10.0
    # the markers follow the model: vertex + T_R o (+ the same 1 mm noise as the plain capture)
    d = off.markers.get_points() - plain.markers.get_points()
    seen = (plain.markers.get_points() != 0).any(-1)
    assert np.abs(d[seen]).max() < 0.03 and np.abs(d[seen]).max() > 1e-3
