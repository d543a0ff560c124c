"""EXTENSION: the Geman-McClure (GMoF) data terms -- C ABI layout, config validation and the Python rho / rho' helpers.  No
GPU needed (tests/test_gpu_robust.py holds the closures)."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_problem_struct_ends_with_robust_sigma_and_matches_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    names = [f[0] for f in _lib.UuoProblem._fields_]
    assert names[-1] == "robust_sigma" and names[-2] == "d_bary"
    assert _lib.UuoProblem._fields_[-1][1] is ctypes.c_float
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uuo_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(uuo_problem_t), offsetof(uuo_problem_t, robust_sigma)); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(_lib.UuoProblem)
    assert off == _lib.UuoProblem.robust_sigma.offset
    assert _lib.ABI_VERSION == 3
    assert _lib.UuoProblem().robust_sigma == 0.0   # a fresh structure is the reference's square


def _cfg(**stage_keys):
    from uuo_mocap_amd.config import packaged_config

    cfg = packaged_config("video_mocap")
    for stage, kv in stage_keys.items():
        cfg["stages"][stage].update(kv)
    return cfg


@pytest.mark.parametrize("stage", ["chamfer", "part", "marker"])
def test_robust_sigma_is_read_and_validated(stage):
    from uuo_mocap_amd.engine import stage_robust_sigma

    assert stage_robust_sigma(_cfg(), stage) == 0.0                                  # absent: off
    assert stage_robust_sigma(_cfg(**{stage: {"robust_sigma": 0}}), stage) == 0.0
    assert stage_robust_sigma(_cfg(**{stage: {"robust_sigma": 0.05}}), stage) == pytest.approx(0.05)
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="robust_sigma"):
            stage_robust_sigma(_cfg(**{stage: {"robust_sigma": bad}}), stage)


@pytest.mark.parametrize("stage", ["chamfer", "part"])
def test_robust_sigma_with_the_soft_assignment_term_is_refused(stage):
    from uuo_mocap_amd.engine import stage_robust_sigma

    losses = dict(_cfg()["stages"][stage]["losses"])
    losses["soft_chamfer"] = 10.0
    cfg = _cfg(**{stage: {"robust_sigma": 0.05, "losses": losses}})
    with pytest.raises(NotImplementedError, match="soft_chamfer"):
        stage_robust_sigma(cfg, stage)
    cfg["stages"][stage]["robust_sigma"] = 0.0
    assert stage_robust_sigma(cfg, stage) == 0.0   # the soft term alone stays available


def test_problem_constructors_refuse_bad_sigma_before_touching_a_device():
    """ChamferProblem / MarkerProblem / PartProblem validate the key before they build anything (no GPU reached)."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem

    bad = _cfg(chamfer={"robust_sigma": -1.0}, marker={"robust_sigma": -1.0}, part={"robust_sigma": -1.0})
    with pytest.raises(ValueError, match="robust_sigma"):
        ChamferProblem(None, None, None, None, None, bad)
    with pytest.raises(ValueError, match="robust_sigma"):
        MarkerProblem(None, None, None, None, None, bad)
    with pytest.raises(ValueError, match="robust_sigma"):
        PartProblem(None, None, None, None, None, None, bad)


def test_execution_switch_and_packaged_config():
    from uuo_mocap_amd.config import packaged_config
    from uuo_mocap_amd.markers_utils import EXECUTION_DEFAULTS, merge_execution
    from uuo_mocap_amd.optimization import lockstep_supported

    assert EXECUTION_DEFAULTS["robust_fused"] is True
    assert merge_execution({"execution": {"robust_fused": False}})["robust_fused"] is False
    cfg = packaged_config("video_mocap_robust")
    base = packaged_config("video_mocap")
    for stage in ("chamfer", "part", "marker"):
        assert cfg["stages"][stage]["robust_sigma"] == 0.1
        assert cfg["stages"][stage]["losses"] == base["stages"][stage]["losses"]
    # the fused closures carry the term, so lock-step batches keep working; the composed route cannot be batched
    assert lockstep_supported(cfg, "chamfer") and lockstep_supported(cfg, "marker")
    cfg["execution"] = {"robust_fused": False}
    assert not lockstep_supported(cfg, "chamfer") and not lockstep_supported(cfg, "marker")
    assert lockstep_supported(dict(base, execution={"robust_fused": False}), "chamfer")   # nothing robust: unaffected


@pytest.mark.parametrize("sigma", [0.01, 0.05, 1.0])
def test_gmof_and_its_derivative_match_float64_autograd(sigma):
    from uuo_mocap_amd.losses import gmof, gmof_grad

    s = torch.cat([torch.logspace(-8, 1, 200, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)]).requires_grad_(True)
    sig2 = sigma * sigma
    ref = s * sig2 / (sig2 + s)
    (g_ref,) = torch.autograd.grad(ref.sum(), s)
    out = gmof(s, sigma)
    (g_out,) = torch.autograd.grad(out.sum(), s)
    torch.testing.assert_close(out, ref, rtol=1e-14, atol=0.0)
    torch.testing.assert_close(g_out, g_ref, rtol=1e-10, atol=1e-18)
    torch.testing.assert_close(gmof_grad(s.detach(), sigma), g_ref, rtol=1e-10, atol=1e-18)
    # limits: ~ s for s << sigma^2, -> sigma^2 for s >> sigma^2, bounded by sigma^2 everywhere
    small = torch.tensor([1e-6 * sig2], dtype=torch.float64)
    assert float(gmof(small, sigma) / small) == pytest.approx(1.0, abs=2e-6)
    assert float(gmof(torch.tensor([1e6 * sig2], dtype=torch.float64), sigma)) == pytest.approx(sig2, rel=2e-6)
    assert float(out.max()) <= sig2


def test_gmof_off_is_the_identity():
    from uuo_mocap_amd.losses import gmof, gmof_grad

    s = torch.rand(17, dtype=torch.float32)
    assert gmof(s, 0.0) is s
    assert torch.equal(gmof_grad(s, 0.0), torch.ones_like(s))
