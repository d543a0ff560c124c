"""EXTENSION: the joint-acceleration smoothness term (stages.{chamfer,marker}.losses.joint_accel) -- config validation, the
composed route's torch term against a numpy restatement, the acceleration-error metric and the C entry point's binding.  No
GPU needed (tests/test_gpu_temporal.py holds the fused closures and the fits)."""
import os
import re
import subprocess
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(name="video_mocap", **stage_losses):
    from uuo_mocap_amd.config import packaged_config

    cfg = packaged_config(name)
    for stage, kv in stage_losses.items():
        cfg["stages"][stage]["losses"].update(kv)
    return cfg


# ------------------------------------------------------------------------------------------------ config validation
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_joint_accel_is_read_and_validated(stage):
    from uuo_mocap_amd.engine import stage_joint_accel

    assert stage_joint_accel(_cfg(), stage) == 0.0                                     # absent: off
    assert stage_joint_accel(_cfg(**{stage: {"joint_accel": 0}}), stage) == 0.0
    assert stage_joint_accel(_cfg(**{stage: {"joint_accel": None}}), stage) == 0.0
    assert stage_joint_accel(_cfg(**{stage: {"joint_accel": 2.5}}), stage) == pytest.approx(2.5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="joint_accel"):
            stage_joint_accel(_cfg(**{stage: {"joint_accel": bad}}), stage)


def test_stage_problems_refuse_bad_weights_before_touching_the_device():
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    with pytest.raises(ValueError, match="joint_accel"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"joint_accel": -2.0}))
    with pytest.raises(ValueError, match="joint_accel"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"joint_accel": float("nan")}))
    with pytest.raises(NotImplementedError, match="soft"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"joint_accel": 1.0, "soft_chamfer": 10.0}))


def test_joint_accel_in_the_part_stage_is_refused():
    from uuo_mocap_amd.engine import PartProblem

    with pytest.raises(NotImplementedError, match="joint_accel"):
        PartProblem(None, None, None, None, None, None, _cfg(part={"joint_accel": 1.0}))


def test_reference_temporal_terms_stay_refused():
    from uuo_mocap_amd.engine import MarkerProblem
    from uuo_mocap_amd.optimization import _optim_chamfer_general

    with pytest.raises(NotImplementedError, match="root_orient_vel"):
        _optim_chamfer_general(None, None, None, None, None, None, None, None, None,
                               _cfg(chamfer={"root_orient_vel": 1.0}), 0, 0, False, None)
    with pytest.raises(NotImplementedError, match="temporal"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"temporal": 1.0}))


def test_routing_flags():
    from uuo_mocap_amd.optimization import lockstep_supported
    from uuo_mocap_amd.terms import FOOT_LOCK, JOINT_ACCEL, StageTerms

    _temporal_fused = lambda cfg, stage: all(StageTerms(cfg, stage).fused(t) for t in (JOINT_ACCEL, FOOT_LOCK))  # one switch for both

    plain, smooth = _cfg(), _cfg("video_mocap_smooth")
    for stage in ("chamfer", "marker"):
        assert lockstep_supported(plain, stage)
        assert lockstep_supported(_cfg(**{stage: {"joint_accel": 0.0}}), stage)
        assert not lockstep_supported(smooth, stage)          # lock-step batches do not carry the term
        assert _temporal_fused(smooth, stage)
        smooth_c = _cfg("video_mocap_smooth")
        smooth_c["execution"] = {"temporal_fused": False}
        assert not _temporal_fused(smooth_c, stage)
        assert _temporal_fused(dict(plain, execution={"temporal_fused": False}), stage)  # nothing to compose without the term


def test_shipped_smooth_config_differs_from_its_parent_only_by_the_term():
    from uuo_mocap_amd.engine import stage_joint_accel

    plain, smooth = _cfg(), _cfg("video_mocap_smooth")
    assert stage_joint_accel(smooth, "chamfer") > 0.0 and stage_joint_accel(smooth, "marker") > 0.0
    assert "joint_accel" not in smooth["stages"]["part"]["losses"]
    for stage in ("chamfer", "marker"):
        rest = {k: v for k, v in smooth["stages"][stage]["losses"].items() if k != "joint_accel"}
        assert rest == plain["stages"][stage]["losses"]
    strip = lambda c: {k: v for k, v in c.items() if k not in ("stages", "name", "parent")}
    assert strip(smooth) == strip(plain)


def test_frame_sharding_refuses_the_term():
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.optimization import optim_chamfer

    F, M = 6, 4
    markers = torch.zeros(F, M, 3)
    z = lambda *s: torch.zeros(*s)
    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="frame-block sharding"):
            optim_chamfer(markers, z(F, 23, 3, 3), z(F, 23, 3, 3), z(1, 10), z(1, 10), z(F, 1, 3, 3), z(F, 3), z(F),
                          torch.zeros(F, M, dtype=torch.long), None, _cfg("video_mocap_smooth"))


# ------------------------------------------------------------------------------------------------ the composed term
def _np_accel(j):
    """numpy restatement: w-free term sum_t |J_t - 2 J_{t+1} + J_{t+2}|^2 / ((F - 2) 3 J), and its gradient."""
    F = j.shape[0]
    if F < 3:
        return 0.0, np.zeros_like(j)
    n = (F - 2) * j.shape[1] * j.shape[2]
    a = np.stack([j[t] - 2 * j[t + 1] + j[t + 2] for t in range(F - 2)])
    g = np.zeros_like(j)
    for f in range(F):
        for t, c in ((f - 2, 1.0), (f - 1, -2.0), (f, 1.0)):
            if 0 <= t <= F - 3:
                g[f] += 2.0 * c * a[t] / n
    return float((a ** 2).sum() / n), g


@pytest.mark.parametrize("F", [2, 3, 4, 9])
def test_composed_term_matches_a_numpy_restatement(F):
    from uuo_mocap_amd.losses import joint_accel_loss

    rng = np.random.default_rng(F)
    j = rng.normal(size=(F, 24, 3)) * 0.3 + np.arange(F)[:, None, None] * 0.01
    jt = torch.tensor(j, requires_grad=True)
    loss = joint_accel_loss(jt)
    loss.backward()
    lo, g = _np_accel(j)
    assert float(loss) == pytest.approx(lo, rel=1e-12, abs=0.0)
    np.testing.assert_allclose(jt.grad.numpy(), g, rtol=1e-10, atol=1e-15)
    if F < 3:
        assert float(loss) == 0.0 and not jt.grad.any()
    else:  # the formula of the issue: F.mse_loss of the second differences
        a = jt.detach()[:-2] - 2 * jt.detach()[1:-1] + jt.detach()[2:]
        assert float(loss) == pytest.approx(float(torch.nn.functional.mse_loss(a, torch.zeros_like(a))), rel=1e-12)


def test_composed_term_is_blind_to_constant_velocity():
    from uuo_mocap_amd.losses import joint_accel_loss

    j0, v = torch.randn(1, 24, 3, dtype=torch.float64), torch.randn(1, 24, 3, dtype=torch.float64)
    traj = j0 + torch.arange(11, dtype=torch.float64)[:, None, None] * v
    assert float(joint_accel_loss(traj)) < 1e-26


# ------------------------------------------------------------------------------------------------ metric
def test_accel_error_known_answers():
    from uuo_mocap_amd.metrics import compute_accel_error

    F, J, freq = 12, 24, 30.0
    t = torch.arange(F, dtype=torch.float64)[:, None, None] / freq
    acc = torch.randn(1, J, 3, dtype=torch.float64)
    x = torch.randn(1, J, 3, dtype=torch.float64) + t * torch.randn(1, J, 3, dtype=torch.float64) + 0.5 * acc * t ** 2
    assert float(compute_accel_error(x, x, freq)) == 0.0
    # constant acceleration: a shifted copy of the same motion has the same acceleration
    assert float(compute_accel_error(x + 0.3, x, freq)) < 1e-9
    # a known value: a bump of h on one frame and joint changes that joint's second differences by h, -2h, h around it
    y = x.clone()
    h = 0.002
    y[5, 7, 1] += h
    expect = (h + 2 * h + h) * freq ** 2 / ((F - 2) * J)
    assert float(compute_accel_error(y, x, freq)) == pytest.approx(expect, rel=1e-9)
    # against constant-acceleration ground truth the error is |acc_pred - acc_gt| in m/s^2
    z = x + 0.5 * torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64) * t ** 2
    assert float(compute_accel_error(z, x, freq)) == pytest.approx(2.0, rel=1e-9)
    with pytest.raises(ValueError):
        compute_accel_error(x[:2], x[:2], freq)


# ------------------------------------------------------------------------------------------------ C entry point
def test_entry_point_is_declared_bound_and_typed_as_in_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    assert "uuo_fit_set_joint_accel" in _lib.header_symbols()
    assert _lib._SIGNATURES["uuo_fit_set_joint_accel"] == (c_int, [c_void_p, c_float])
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+uuo_fit_set_joint_accel\s*\(\s*uuo_fit_t\s*\*\s*fit\s*,\s*float\s+w\s*\)\s*;", text)
    src = tmp_path / "sig.c"
    src.write_text('#include "uuo_hip.h"\nint (*fp)(uuo_fit_t*, float) = uuo_fit_set_joint_accel;\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "sig.o")])
    # the problem structure did not grow (the ABI of tests/test_robust_terms.py)
    assert [f[0] for f in _lib.UuoProblem._fields_][-1] == "robust_sigma" and _lib.ABI_VERSION == 3


def test_units_note_in_the_header():
    from uuo_mocap_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    assert "uuo_fit_set_joint_accel" in text and "frame rate" in text
