"""The root stage (optim_root: translation, yaw and shape with the body pose held) without a GPU: the ABI's new values, the
parameter counts, every refusal -- raised on host tensors, before a device is touched -- and the float64 restatement of the
closure (root_ref64) against central finite differences."""
import copy
import ctypes
import re
import types

import numpy as np
import pytest
import torch

from gpu_support import _inputs, smpl64  # noqa: F401  (fixture)
from root_ref64 import ref_root64
from uuo_mocap_amd import _lib, engine, optimization, parallel, terms
from uuo_mocap_amd.config import packaged_config


def _cfg(**root):
    cfg = copy.deepcopy(packaged_config("video_mocap_root"))
    cfg["stages"]["root"].update(root)
    return cfg


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_names_both_stages_and_the_library_exports_the_setter():
    header = open(_lib.HEADER_PATH).read()
    values = dict(re.findall(r"\b(UUO_STAGE_[A-Z_]+) = (\d+)", header))
    assert values == {"UUO_STAGE_CHAMFER": "0", "UUO_STAGE_MARKER": "1", "UUO_STAGE_PART": "2", "UUO_STAGE_ROOT": "4",
                      "UUO_STAGE_ROOT_SHARED": "5"}
    assert (_lib.UUO_STAGE_ROOT, _lib.UUO_STAGE_ROOT_SHARED) == (4, 5)
    assert "uuo_fit_set_root_trans_vel" in _lib.header_symbols()
    assert re.search(r"int uuo_fit_set_root_trans_vel\(uuo_fit_t\* fit, float w\);", header)
    res, args = _lib._SIGNATURES["uuo_fit_set_root_trans_vel"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_float]
    lib = _lib.load()   # (checks every symbol of the header)
    assert hasattr(lib, "uuo_fit_set_root_trans_vel")
    assert lib.uuo_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.parametrize("F", [1, 2, 7])
def test_parameter_counts(F):
    lib = _lib.load()

    def n(stage, **kw):
        p = _lib.UuoProblem()
        p.stage, p.F, p.M = stage, F, 3
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.uuo_problem_num_params(ctypes.byref(p))

    assert n(_lib.UUO_STAGE_ROOT) == 4 * F + 10
    assert n(_lib.UUO_STAGE_ROOT_SHARED) == 3 * F + 11
    assert (n(0), n(1), n(2)) == (211 * F + 10, 219 * F + 10, 3 * F + 11)   # the three old stages: what they gave
    assert n(1, w_offsets=1.0) == 219 * F + 10 + 9
    assert n(3) == -22 and n(6) == -22 and n(-1) == -22                      # 3 stays internal


# ------------------------------------------------------------------------------------------------ refusals, on the host
def _host_call(cfg, **kw):
    F, M = 3, 4
    args = dict(markers=torch.ones(F, M, 3), pose_body=torch.eye(3).expand(F, 23, 3, 3).clone(), betas=torch.zeros(1, 10),
                root_orient=torch.eye(3).expand(F, 1, 3, 3).clone(), trans=torch.zeros(F, 3), marker_labels=None,
                smpl_inference=None, config=cfg)
    args.update(kw)
    return optimization.optim_root(**args)


_EXTENSION_LOSS_KEYS = sorted(set().union(*(t.keys for t in terms.TERMS)) | {"soft_chamfer", "surface_chamfer"})


@pytest.mark.parametrize("key", ["root_orient_vel", "ground", "part_chamfer"] + _EXTENSION_LOSS_KEYS)
def test_refused_loss_keys_name_the_key(key):
    cfg = _cfg()
    cfg["stages"]["root"]["losses"][key] = 1.0
    with pytest.raises(NotImplementedError, match=re.escape(key)):
        _host_call(cfg)
    with pytest.raises(NotImplementedError, match=re.escape(key)):
        engine.RootProblem(None, torch.ones(3, 4, 3), None, None, None, cfg)


def test_every_extension_key_of_the_term_table_is_covered():
    assert {"joint_accel", "latent_offsets", "foot_lock", "floor_penetration", "floor_contact", "self_penetration", "joint_limits",
            "pose_gmm", "keypoints_2d", "pose_accel"} <= set(_EXTENSION_LOSS_KEYS)


@pytest.mark.parametrize("key,value", [("robust_sigma", 0.1), ("prior_confidence", {"gap_weight": 0.0})])
def test_refused_stage_keys_name_the_key(key, value):
    with pytest.raises(NotImplementedError, match=key):
        _host_call(_cfg(**{key: value}))


def test_refused_modes():
    with pytest.raises(NotImplementedError, match="yaw_lock.*constrained_rotation"):
        _host_call(_cfg(yaw_lock=False, constrained_rotation=False))
    with pytest.raises(NotImplementedError, match="single_directional"):
        _host_call(_cfg(single_directional=False))
    with pytest.raises(NotImplementedError, match="host tensors"):
        _host_call(_cfg())
    with pytest.raises(NotImplementedError, match="host tensors"):
        _host_call(_cfg(constrained_rotation=True))
    assert engine.root_stage_settings(_cfg(constrained_rotation=True, yaw_lock=False))["shared"] is True   # tested first
    assert engine.root_stage_settings(_cfg())["shared"] is False


def test_refused_sharding_shared_betas_and_lockstep(monkeypatch):
    monkeypatch.setattr(parallel._ctx, "frames", types.SimpleNamespace(active=True), raising=False)
    with pytest.raises(NotImplementedError, match="frame sharding"):
        _host_call(_cfg())
    monkeypatch.setattr(parallel._ctx, "frames", None, raising=False)
    monkeypatch.setattr(parallel._ctx, "shared", object(), raising=False)
    with pytest.raises(NotImplementedError, match="shared betas"):
        _host_call(_cfg())
    monkeypatch.setattr(parallel._ctx, "shared", None, raising=False)
    for stage in (_lib.UUO_STAGE_ROOT, _lib.UUO_STAGE_ROOT_SHARED):
        stand_in = types.SimpleNamespace(stage=stage, model=None, F=3, M=4)
        with pytest.raises(NotImplementedError, match="lock-step batches do not carry the root stage"):
            engine.solve_batch([stand_in], [None], max_iter=1)


def test_settings_defaults():
    cfg = _cfg()
    del cfg["stages"]["root"]["lr"]
    s = engine.root_stage_settings(cfg)
    assert s["lr"] == 0.1 and s["w_data"] == 10.0 and s["w_betas"] == 0.1 and s["w_tvel"] == 0.0   # an absent key means 0
    cfg["stages"]["root"]["losses"] = {"trans_vel": 2.0}
    s = engine.root_stage_settings(cfg)
    assert (s["w_data"], s["w_betas"], s["w_tvel"]) == (0.0, 0.0, 2.0)
    assert packaged_config("video_mocap_root")["find_best_part_fits"] is False
    assert packaged_config("video_mocap")["stages"]["root"]["num_iters"] == 0


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shared", [False, True])
def test_ref_root64_agrees_with_central_differences(tables, smpl64, shared):  # noqa: F811
    """F = 3, M = 5, one marker missing, trans_vel on, the assignment held: the autograd gradient of the float64 restatement
    against (f(x + h e) - f(x - h e)) / 2h, h = 1e-6.  The closure is smooth in x at a held assignment, so the difference's
    error is h^2 f''' / 6 + eps f / h ~ 1e-10 relative to entries of order 1; 1e-6 of the gradient's norm leaves room."""
    F, M = 3, 5
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 41, M)
    markers = markers.clone()
    markers[markers.abs().sum(-1) == 0] = 0.3   # (every entry present, then exactly one missing)
    markers[1, 2] = 0.0
    cfg = _cfg()
    cfg["stages"]["root"]["losses"]["trans_vel"] = 3.0
    z = zp[:1] if shared else zp
    x = torch.cat([tp.reshape(-1), z.reshape(-1), bp.reshape(-1)]).double()
    assert x.numel() == (3 * F + 11 if shared else 4 * F + 10)
    gen = torch.Generator().manual_seed(3)
    nn = torch.randint(0, 6890, (F, M), generator=gen)
    args = (smpl64, cfg, markers, o_pose, o_betas, root)
    loss, grad = ref_root64(*args, x, nn, shared)
    assert np.isfinite(loss) and loss > 0.0 and grad.shape == (x.numel(),)
    h = 1e-6
    fd = np.zeros_like(grad)
    for i in range(x.numel()):
        e = torch.zeros_like(x)
        e[i] = h
        fd[i] = (ref_root64(*args, x + e, nn, shared)[0] - ref_root64(*args, x - e, nn, shared)[0]) / (2.0 * h)
    assert np.linalg.norm(grad - fd) < 1e-6 * np.linalg.norm(grad), (np.linalg.norm(grad - fd), np.linalg.norm(grad))
    # every block is live: translation (data and trans_vel), yaw, shape
    nz = 1 if shared else F
    for sl in (slice(0, 3 * F), slice(3 * F, 3 * F + nz), slice(3 * F + nz, None)):
        assert np.linalg.norm(grad[sl]) > 0.0
    # the missing marker carries nothing: moving its assignment changes neither the loss nor the gradient
    nn2 = nn.clone()
    nn2[1, 2] = (int(nn[1, 2]) + 1) % 6890
    loss2, grad2 = ref_root64(*args, x, nn2, shared)
    assert loss2 == loss and np.array_equal(grad2, grad)
