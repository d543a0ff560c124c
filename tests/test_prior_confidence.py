"""EXTENSION: per-(frame, joint) weights on the video pose prior (stages.{chamfer,marker}.prior_confidence,
uuo_fit_set_prior_weights) -- config validation and routing, the weight table against a loop restatement, the video mask's way to
the mocap frames, the composed route's term against float64 numpy and difference quotients, the generator's dropout capture,
the metric and the C entry point's binding.  No GPU needed (tests/test_gpu_prior_confidence.py holds the fused closures and the
fits)."""
import os
import re
import subprocess
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
BLOCK = {"gap_weight": 0.3, "ramp": 2, "joint_weights": None}


def _cfg(name="video_mocap", **stages):
    """packaged config; per stage a dict whose `prior_confidence` entry goes on the stage, the rest on its losses"""
    from uuo_mocap_amd.config import packaged_config

    cfg = packaged_config(name)
    for stage, kv in stages.items():
        for k, v in kv.items():
            if k == "prior_confidence":
                cfg["stages"][stage]["prior_confidence"] = v
            else:
                cfg["stages"][stage]["losses"][k] = v
    return cfg


# ------------------------------------------------------------------------------------------------ 1. config, refusals, routing
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_block_is_read_and_validated(stage):
    from uuo_mocap_amd.engine import stage_prior_confidence

    assert stage_prior_confidence(_cfg(), stage) is None                                     # absent: off
    assert stage_prior_confidence(_cfg(**{stage: {"prior_confidence": None}}), stage) is None  # null: off
    assert stage_prior_confidence(_cfg(**{stage: {"prior_confidence": {}}}), stage) == \
        {"gap_weight": 0.0, "ramp": 0, "joint_weights": None}
    jw = [0.5] * 22 + [2.0]
    got = stage_prior_confidence(_cfg(**{stage: {"prior_confidence": {"gap_weight": 1, "ramp": 5, "joint_weights": jw}}}), stage)
    assert got == {"gap_weight": 1.0, "ramp": 5, "joint_weights": jw}
    other = "marker" if stage == "chamfer" else "chamfer"
    assert stage_prior_confidence(_cfg(**{stage: {"prior_confidence": dict(BLOCK)}}), other) is None   # per stage
    bad = [{"gap_weight": -0.1}, {"gap_weight": 1.5}, {"gap_weight": float("nan")}, {"gap_weight": INF}, {"gap_weight": "0.1"},
           {"gap_weight": True}, {"ramp": -1}, {"ramp": 1.5}, {"ramp": 2.0}, {"ramp": True}, {"ramp": None},
           {"joint_weights": [1.0] * 22}, {"joint_weights": [1.0] * 22 + [-0.5]}, {"joint_weights": [1.0] * 22 + [INF]},
           {"joint_weights": [1.0] * 22 + [float("nan")]}, {"joint_weights": 1.0}, {"weights": 1.0}, dict(BLOCK, extra=1),
           [0.0, 0], "on"]
    for b in bad:
        with pytest.raises(ValueError, match="prior_confidence"):
            stage_prior_confidence(_cfg(**{stage: {"prior_confidence": b}}), stage)
    # a block beside a reg_pose_body that is absent or 0 is allowed
    cfg = _cfg(**{stage: {"prior_confidence": dict(BLOCK), "reg_pose_body": 0.0}})
    assert stage_prior_confidence(cfg, stage) == BLOCK
    del cfg["stages"][stage]["losses"]["reg_pose_body"]
    assert stage_prior_confidence(cfg, stage) == BLOCK


def test_bad_values_raise_before_the_device_is_touched():
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, check_prior_weights

    with pytest.raises(ValueError, match="prior_confidence"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"prior_confidence": {"gap_weight": 2.0}}))
    with pytest.raises(ValueError, match="prior_confidence"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"prior_confidence": {"ramp": -3}}))
    with pytest.raises(ValueError, match="prior_weights"):
        ChamferProblem(None, None, None, None, None, _cfg(), prior_weights=torch.ones(5, 22))
    with pytest.raises(ValueError, match="prior_weights"):
        MarkerProblem(None, None, None, None, None, _cfg(), prior_weights=-torch.ones(5, 23))
    with pytest.raises(NotImplementedError, match="soft"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"soft_chamfer": 10.0}), prior_weights=torch.zeros(5, 23))
    assert check_prior_weights(None) is None
    w = check_prior_weights(np.full((4, 23), 0.5), 4)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4, 23)
    for bad in (torch.ones(4, 23, 1), torch.ones(3, 23), torch.full((4, 23), float("nan")), torch.full((4, 23), INF),
                torch.full((4, 23), -1e-3)):
        with pytest.raises(ValueError, match="prior_weights"):
            check_prior_weights(bad, 4)


def test_routing_flags():
    from uuo_mocap_amd.optimization import _stage_terms, lockstep_supported
    from uuo_mocap_amd.terms import PRIOR, StageTerms

    _prior_conf_on = lambda cfg, stage: StageTerms(cfg, stage).on(PRIOR)
    _armed_prior_weights = lambda cfg, stage, weights, num_frames: _stage_terms(cfg, stage, weights, num_frames).prior_weights

    plain, drop = _cfg(), _cfg("video_mocap_dropout")
    half = torch.full((6, 23), 0.5)
    for stage in ("chamfer", "marker"):
        assert not _prior_conf_on(plain, stage) and _prior_conf_on(drop, stage)
        assert lockstep_supported(plain, stage) and not lockstep_supported(drop, stage)   # lock-step batches do not carry it
        assert lockstep_supported(_cfg(**{stage: {"prior_confidence": None}}), stage)
        assert _armed_prior_weights(drop, stage, None, 6) is None
        assert _armed_prior_weights(drop, stage, torch.ones(6, 23), 6) is None            # ones arm nothing
        assert torch.equal(_armed_prior_weights(plain, stage, half, 6), half)
        with pytest.raises(ValueError, match="prior_weights"):
            _armed_prior_weights(plain, stage, half, 7)
        composed = dict(drop, execution={"prior_conf_fused": False})
        _prior_conf_fused = lambda cfg, weights: StageTerms(cfg, stage, weights).fused(PRIOR)
        assert _prior_conf_fused(drop, half) and not _prior_conf_fused(composed, half)
        assert _prior_conf_fused(composed, None)                                           # nothing to compose without weights


def _zeros(*s):
    return torch.zeros(*s)


class _Smpl:
    class device_model:
        V = 6890


def _stage_args(F, M):
    markers = _zeros(F, M, 3)
    one_hot = _zeros(M, 6890)
    one_hot[:, 0] = 1.0
    args_c = (markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3), _zeros(F, 3),
              _zeros(F), torch.zeros(F, M, dtype=torch.long), None)
    args_m = (markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3),
              _zeros(F, 3), one_hot, _zeros(F), _Smpl)
    return args_c, args_m


def test_composed_routes_are_taken(monkeypatch):
    """execution.prior_conf_fused: False with armed weights, and soft_chamfer + armed weights, go to the closures composed from
    the operators, which receive the checked table; ones or None stay on the fused route"""
    from uuo_mocap_amd import optimization as opt

    F, M = 6, 4
    args_c, args_m = _stage_args(F, M)
    taken = []
    monkeypatch.setattr(opt, "_optim_chamfer_general", lambda *a, **k: taken.append(("chamfer", a[-1])))
    monkeypatch.setattr(opt, "_optim_markers_general", lambda *a, **k: taken.append(("marker", a[-1])))
    cfg = _cfg("video_mocap_dropout")
    cfg["execution"] = {"prior_conf_fused": False}
    w = torch.full((F, 23), 0.25)
    opt.optim_chamfer(*args_c, cfg, prior_weights=w)
    opt.optim_markers(*args_m, cfg, prior_weights=w)
    assert [t[0] for t in taken] == ["chamfer", "marker"] and all(torch.equal(t[1], w) for t in taken)
    soft = _cfg("video_mocap_dropout", chamfer={"soft_chamfer": 10.0})
    opt.optim_chamfer(*args_c, soft, prior_weights=w)   # (markers on the host: the fused soft closure is not in reach either way)
    assert len(taken) == 3 and torch.equal(taken[2][1], w)

    class _Stop(Exception):
        pass

    def stop(*a, **k):
        assert k.get("prior_weights") is None     # ones / None arm nothing
        raise _Stop()

    monkeypatch.setattr(opt, "ChamferProblem", stop)
    monkeypatch.setattr(opt, "MarkerProblem", stop)
    for pw in (None, torch.ones(F, 23)):
        with pytest.raises(_Stop):
            opt.optim_chamfer(*args_c, cfg, prior_weights=pw)
        with pytest.raises(_Stop):
            opt.optim_markers(*args_m, cfg, prior_weights=pw)
    assert len(taken) == 3


def test_frame_sharding_refuses_the_weights():
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.optimization import optim_chamfer, optim_markers

    F, M = 6, 4
    args_c, args_m = _stage_args(F, M)
    w = torch.full((F, 23), 0.25)
    with parallel.shard_frames(joint_with_one_rank=True):
        for cfg, pw in ((_cfg("video_mocap_dropout"), None), (_cfg(), w)):   # the block, or an armed table
            with pytest.raises(NotImplementedError, match="prior_confidence.*frame-block sharding"):
                optim_chamfer(*args_c, cfg, prior_weights=pw)
            with pytest.raises(NotImplementedError, match="prior_confidence.*frame-block sharding"):
                optim_markers(*args_m, cfg, prior_weights=pw)


def test_solve_batch_refuses_the_weights_up_front():
    from uuo_mocap_amd.engine import solve_batch

    class _P:
        model = None
        joint_accel = 0.0
        foot_lock = 0.0
        floor_on = False
        capsules_on = False
        joint_limits_on = False
        prior_conf_on = True

        class problem:
            w_offsets = 0.0

    with pytest.raises(NotImplementedError, match="prior_confidence"):
        solve_batch([_P()], [None], max_iter=1)


def test_shipped_config_differs_from_its_parent_only_by_the_block():
    from uuo_mocap_amd.engine import stage_prior_confidence

    plain, drop = _cfg(), _cfg("video_mocap_dropout")
    for stage in ("chamfer", "marker"):
        blk = stage_prior_confidence(drop, stage)
        assert blk is not None and blk["joint_weights"] is None and 0.0 <= blk["gap_weight"] <= 1.0
        assert {k: v for k, v in drop["stages"][stage].items() if k != "prior_confidence"} == plain["stages"][stage]
    for k in plain["stages"]:
        if k not in ("chamfer", "marker"):
            assert drop["stages"][k] == plain["stages"][k]
    assert {k: v for k, v in drop.items() if k not in ("stages", "name", "parent")} == \
        {k: v for k, v in plain.items() if k not in ("stages", "name", "parent")}


# ------------------------------------------------------------------------------------------------ 2. the weight table
def _table_loops(seen, gap_weight, ramp, joint_weights):
    """the issue's definition, loops"""
    F = len(seen)
    out = np.zeros((F, 23), dtype=np.float32)
    for t in range(F):
        d = min(abs(t - u) for u in range(F) if seen[u])
        fw = 1.0 if d == 0 else max(gap_weight, 1.0 - d / (ramp + 1.0))
        for j in range(23):
            out[t, j] = np.float32(fw * (1.0 if joint_weights is None else joint_weights[j]))
    return out


JOINT_TABLE = [1.0] * 23
JOINT_TABLE[3], JOINT_TABLE[17] = 0.0, 1.75   # a zero and a value above 1


def _mask(F, gaps):
    m = np.ones(F, dtype=bool)
    for a, b in gaps:
        m[a:b] = False
    return m


MASKS = {"leading": _mask(20, [(0, 7)]), "interior": _mask(20, [(6, 15)]), "trailing": _mask(20, [(12, 20)]),
         "all three": _mask(40, [(0, 4), (10, 23), (33, 40)]), "single seen frame": _mask(9, [(0, 4), (5, 9)])}


@pytest.mark.parametrize("ramp", [0, 2, 5])
@pytest.mark.parametrize("gap_weight", [0.0, 0.3])
def test_weight_table_matches_the_loop_restatement(ramp, gap_weight):
    from uuo_mocap_amd.engine import prior_weight_table

    for name, mask in MASKS.items():
        for jw in (None, JOINT_TABLE):
            blk = {"gap_weight": gap_weight, "ramp": ramp, "joint_weights": jw}
            for seen in (torch.from_numpy(mask), mask, mask.astype(np.float32)):
                got = prior_weight_table(seen, blk)
                assert got.dtype == torch.float32 and tuple(got.shape) == (len(mask), 23), name
                assert np.array_equal(got.numpy(), _table_loops(mask, gap_weight, ramp, jw)), (name, jw is None)
            assert bool((got[torch.from_numpy(mask)] == torch.tensor(jw or [1.0] * 23)).all())   # seen frames: the joints' own
            if jw is not None:
                assert not got[:, 3].any() and float(got[:, 17].max()) == 1.75
    with pytest.raises(ValueError, match="no frame"):
        prior_weight_table(torch.zeros(12, dtype=torch.bool), {"gap_weight": gap_weight, "ramp": ramp, "joint_weights": None})


def test_ramp_by_hand():
    from uuo_mocap_amd.engine import prior_weight_table

    seen = torch.tensor([1, 0, 0, 0, 0, 0, 0, 1], dtype=torch.bool)
    col = lambda ramp, gw: prior_weight_table(seen, {"gap_weight": gw, "ramp": ramp, "joint_weights": None})[:, 0].double().numpy()
    np.testing.assert_array_equal(col(0, 0.0), [1, 0, 0, 0, 0, 0, 0, 1])                  # ramp 0: every unseen frame gap_weight
    np.testing.assert_allclose(col(2, 0.0), [1, 2 / 3, 1 / 3, 0, 0, 1 / 3, 2 / 3, 1], rtol=1e-7)   # ramp 2 tapers 2/3, 1/3
    np.testing.assert_allclose(col(2, 0.5), [1, 2 / 3, 0.5, 0.5, 0.5, 0.5, 2 / 3, 1], rtol=1e-7)
    assert torch.equal(prior_weight_table(torch.ones(5), BLOCK), torch.ones(5, 23))       # nothing unseen: ones


# ------------------------------------------------------------------------------------------------ 3. the mask's way to the fit
def test_seen_frames_through_resampling_truncation_and_padding():
    from uuo_mocap_amd.engine import prior_weight_table
    from uuo_mocap_amd.multimodal import seen_mocap_frames
    from uuo_mocap_amd.resample import resample_hmr

    mask = torch.tensor([1, 1, 0, 1, 1], dtype=torch.bool)
    # same rate: truncation to the markers' frames, then pad(offset) repeats the first (offset > 0) or last (< 0) frame
    assert seen_mocap_frames(mask, 30.0, 30.0, 4, 0).tolist() == [True, True, False, True]
    assert seen_mocap_frames(mask, 30.0, 30.0, 9, 2).tolist() == [True, True, True, True, False, True, True]
    assert seen_mocap_frames(mask, 30.0, 30.0, 3, -2).tolist() == [True, True, False, False, False]
    # 30 -> 120 Hz: 20 frames, mocap frame i at video frame i / 4; seen only where both neighbours are, or exactly on a seen
    # video frame (i = 4: on frame 1, next to the unseen frame 2)
    want = [True] * 5 + [False] * 7 + [True] * 8
    assert seen_mocap_frames(mask, 30.0, 120.0, 1000, 0).tolist() == want
    assert seen_mocap_frames(mask, 30.0, 120.0, 14, 1).tolist() == [True] + want[:14]
    # 30 -> 25 Hz: round(5 * 25 / 30) = 4 frames at video times 0, 1.2, 2.4, 3.6
    assert seen_mocap_frames(mask, 30.0, 25.0, 1000, 0).tolist() == [True, False, False, True]
    # ... which is where resample_hmr's lerp of the mask, taken along as a contact column, is exactly 1
    for dst in (120.0, 25.0):
        fc = resample_hmr(torch.zeros(5, 3), torch.eye(3).repeat(5, 1, 1, 1), torch.eye(3).repeat(5, 23, 1, 1),
                          mask.float()[:, None].repeat(1, 2), 30.0, dst)[3]
        assert (fc[:, 0] == 1.0).tolist() == seen_mocap_frames(mask, 30.0, dst, 1000, 0).tolist()
    # the table on top: 30 -> 120 Hz, ramp 2
    tab = prior_weight_table(seen_mocap_frames(mask, 30.0, 120.0, 1000, 0), {"gap_weight": 0.0, "ramp": 2, "joint_weights": None})
    np.testing.assert_allclose(tab[:, 0].double().numpy(), [1] * 5 + [2 / 3, 1 / 3, 0, 0, 0, 1 / 3, 2 / 3] + [1] * 8, rtol=1e-7)
    tab = prior_weight_table(seen_mocap_frames(mask, 30.0, 25.0, 1000, 0), {"gap_weight": 0.25, "ramp": 0, "joint_weights": None})
    assert tab[:, 5].tolist() == [1.0, 0.25, 0.25, 1.0]


# ------------------------------------------------------------------------------------------------ 4. the composed term
def _term_inputs(F, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(F, 23, 3, 3, generator=g, dtype=torch.float64)
    o = raw + 0.1 * torch.randn(F, 23, 3, 3, generator=g, dtype=torch.float64)
    w = 2.0 * torch.rand(F, 23, generator=g, dtype=torch.float64)
    w[0] = 0.0
    w[:, 5] = 0.0
    return raw, o, w


def test_weighted_pose_prior_matches_the_numpy_restatement():
    import torch.nn.functional as Fn

    from uuo_mocap_amd.losses import weighted_pose_prior
    from uuo_mocap_amd.optimization import weighted_mse_loss

    for F in (1, 4):
        raw, o, w = _term_inputs(F, 10 + F)
        want = 0.0
        rn, on, wn = raw.numpy(), o.numpy(), w.numpy()
        for t in range(F):
            for j in range(23):
                want += wn[t, j] * float(((rn[t, j] - on[t, j]) ** 2).sum())
        want /= F * 207.0
        got = weighted_pose_prior(raw, o, w)
        assert float(got) == pytest.approx(want, rel=1e-13)
        assert float(weighted_mse_loss(raw, o, w[:, :, None, None])) == pytest.approx(want, rel=1e-13)   # the reference's helper
        assert float(weighted_pose_prior(raw, o, torch.ones(F, 23))) == pytest.approx(float(Fn.mse_loss(raw, o)), rel=1e-13)
        # float32 inputs with a float32 or float64 table on any device-less path
        g32 = weighted_pose_prior(raw.float(), o.float(), w)
        assert g32.dtype == torch.float32 and float(g32) == pytest.approx(want, rel=1e-5)


def test_gradient_against_the_formula_and_central_differences():
    from uuo_mocap_amd.losses import weighted_pose_prior

    F = 3
    raw, o, w = _term_inputs(F, 99)
    leaf = raw.clone().requires_grad_(True)
    reg = 0.7
    (reg * weighted_pose_prior(leaf, o, w)).backward()
    want = 2.0 * reg / (F * 207.0) * w[:, :, None, None] * (raw - o)
    np.testing.assert_allclose(leaf.grad.numpy(), want.numpy(), rtol=1e-12, atol=1e-18)
    assert not leaf.grad[0].any() and not leaf.grad[:, 5].any()          # weight 0: exact zeros
    h = 1e-6
    flat = raw.reshape(-1)
    for idx in range(0, flat.numel(), 37):
        up, dn = flat.clone(), flat.clone()
        up[idx] += h
        dn[idx] -= h
        q = reg * (float(weighted_pose_prior(up.reshape(raw.shape), o, w)) - float(weighted_pose_prior(dn.reshape(raw.shape), o, w))) / (2 * h)
        assert q == pytest.approx(float(leaf.grad.reshape(-1)[idx]), rel=1e-6, abs=1e-10)


# ------------------------------------------------------------------------------------------------ 5. the dropout capture
@pytest.fixture(scope="module")
def tables():
    from uuo_mocap_amd.body_model import synthetic_smpl

    return synthetic_smpl(0)


@pytest.fixture(scope="module")
def sequences(tables):
    from uuo_mocap_amd.synthetic import make_sequence

    return (make_sequence(tables, seed=0, num_frames=300, num_markers=50),
            make_sequence(tables, seed=0, num_frames=300, num_markers=50, video_dropout=False),
            make_sequence(tables, seed=0, num_frames=300, num_markers=50, video_dropout=True))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_option_off_changes_nothing(sequences):
    base, off, _ = sequences
    assert set(base.gt) == set(off.gt) and not {"dropout_window", "hmr_gap_error"} & set(base.gt)
    for k in base.gt:
        assert _same(base.gt[k], off.gt[k]), k
    for k, v in vars(base.img_smpl).items():
        assert _same(v, getattr(off.img_smpl, k)), k
    assert bool(base.img_smpl.img_mask.all())
    assert np.array_equal(base.markers.get_points(), off.markers.get_points())


def _geodesic(a, b):
    rel = np.einsum("fjab,fjac->fjbc", a.astype(np.float64), b.astype(np.float64))
    return np.arccos(np.clip(0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0), -1.0, 1.0))


def test_dropout_sequence(tables, sequences):
    from uuo_mocap_amd.ingest import fill_gaps
    from uuo_mocap_amd.synthetic import DROPOUT_WINDOW, make_sequence

    base, _, seq = sequences
    t0, t1 = seq.gt["dropout_window"]
    assert DROPOUT_WINDOW == 90 and (t0, t1) == (100, 190)
    mask = seq.img_smpl.img_mask
    assert mask.dtype == torch.bool and not mask[t0:t1].any() and bool(mask[:t0].all()) and bool(mask[t1:].all())
    # markers and ground truth are untouched
    assert np.array_equal(base.markers.get_points(), seq.markers.get_points())
    for k in base.gt:
        assert _same(base.gt[k], seq.gt[k]), k
    # the five tracks: fill_gaps of the stand-in's own neighbours in the window, the stand-in's outside it
    tracks = {k: getattr(base.img_smpl, k) for k in ("trans", "root_orient", "hmr_root_orient", "pose_body", "betas")}
    filled = fill_gaps(tracks, mask)
    out = mask.clone()
    for k, v in tracks.items():
        got = getattr(seq.img_smpl, k)
        assert torch.equal(got, filled[k]), k
        assert torch.equal(got[out], v[out]) and not torch.equal(got[t0:t1], v[t0:t1]), k
    # in the gap the filled pose moves on the arc between its two seen neighbours: by hand for one frame and joint
    a, b = t0 - 1, t1
    alpha = (130 - a) / (b - a)
    ra, rb = (base.img_smpl.pose_body[i, 7].double().numpy() for i in (a, b))
    rel = ra.T @ rb
    ang = np.arccos(np.clip(0.5 * (np.trace(rel) - 1.0), -1.0, 1.0))
    axis = np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]]) / (2.0 * np.sin(ang))
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    want = ra @ (np.eye(3) + np.sin(alpha * ang) * K + (1.0 - np.cos(alpha * ang)) * (K @ K))
    np.testing.assert_allclose(seq.img_smpl.pose_body[130, 7].double().numpy(), want, atol=2e-6)
    np.testing.assert_allclose(seq.img_smpl.trans[130].double().numpy(),
                               ((1 - alpha) * base.img_smpl.trans[a] + alpha * base.img_smpl.trans[b]).double().numpy(), atol=1e-6)
    # contacts are 0 in the window; every other field is what it was
    assert not seq.img_smpl.foot_contacts[t0:t1].any()
    for k, v in vars(base.img_smpl).items():
        if k not in tracks and k != "img_mask":
            assert _same(v, getattr(seq.img_smpl, k)), k
    planted = make_sequence(tables, seed=0, num_frames=300, num_markers=50, planted_feet=True, video_dropout=True)
    planted0 = make_sequence(tables, seed=0, num_frames=300, num_markers=50, planted_feet=True)
    assert planted0.img_smpl.foot_contacts[t0:t1].any() and not planted.img_smpl.foot_contacts[t0:t1].any()
    assert torch.equal(planted.img_smpl.foot_contacts[out], planted0.img_smpl.foot_contacts[out])
    # the reported error, and the demonstration's precondition: the filled target is at least 1.5 x as wrong as the stand-in
    err = seq.gt["hmr_gap_error"]
    assert err.shape == (300,)
    np.testing.assert_allclose(err, _geodesic(seq.gt["rot"][:, 1:], seq.img_smpl.pose_body.numpy()).mean(axis=1), atol=1e-6)
    inside, outside = err[t0:t1].mean(), np.concatenate([err[:t0], err[t1:]]).mean()
    print("OBS dropout capture: filled target %.3f rad in the window, stand-in %.3f rad outside, ratio %.2f"
          % (inside, outside, inside / outside))
    assert inside >= 1.5 * outside
    # the window needs a seen frame on both sides
    for F in (100, 136):    # (F = 136: the window [46, 136) would leave no seen frame behind it)
        with pytest.raises(ValueError, match="video_dropout"):
            make_sequence(tables, seed=0, num_frames=F, num_markers=8, video_dropout=True)
    short = make_sequence(tables, seed=0, num_frames=137, num_markers=8, video_dropout=True)
    assert short.gt["dropout_window"] == (46, 136) and bool(short.img_smpl.img_mask[136])


def test_window_vertex_error_metric():
    from uuo_mocap_amd.metrics import compute_window_vertex_error

    gt = torch.zeros(10, 4, 3)
    pred = torch.zeros(10, 4, 3)
    pred[:, :, 0] = torch.arange(10.0)[:, None]          # frame t is off by t
    got = compute_window_vertex_error(pred, gt, (2, 5))
    assert got["inside"] == pytest.approx(3.0) and got["outside"] == pytest.approx((45.0 - 9.0) / 7.0)
    assert got["all"] == pytest.approx(4.5)
    assert np.isnan(compute_window_vertex_error(pred, gt, (3, 3))["inside"])
    assert np.isnan(compute_window_vertex_error(pred, gt, (0, 10))["outside"])
    for bad in ((5, 2), (0, 11), (-1, 3)):
        with pytest.raises(ValueError, match="window"):
            compute_window_vertex_error(pred, gt, bad)
    with pytest.raises(ValueError, match="F, V, 3"):
        compute_window_vertex_error(pred[:5], gt, (0, 1))


# ------------------------------------------------------------------------------------------------ 6. C entry point
def test_entry_point_is_declared_bound_and_typed_as_in_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    assert "uuo_fit_set_prior_weights" in _lib.header_symbols()
    sig = [c_void_p, c_void_p]
    assert _lib._SIGNATURES["uuo_fit_set_prior_weights"] == (c_int, sig)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+uuo_fit_set_prior_weights\s*\(\s*uuo_fit_t\s*\*\s*fit\s*,\s*const\s+float\s*\*\s*d_weights\s*\)\s*;", text)
    src = tmp_path / "sig.c"
    src.write_text('#include "uuo_hip.h"\nint (*fp)(uuo_fit_t*, const float*) = uuo_fit_set_prior_weights;\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "sig.o")])
    assert _lib.ABI_VERSION == 3  # the problem structure and the ABI version did not change
    lib = _lib.load()             # (dlopen needs no GPU) bound with the declared types
    assert lib.uuo_fit_set_prior_weights.argtypes == sig and lib.uuo_fit_set_prior_weights.restype == c_int


def test_note_in_the_header():
    from uuo_mocap_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    note = text[text.index("a weight per (frame, body joint)"):text.index("int uuo_fit_set_prior_weights")]
    assert "EXTENSION" in text[text.index("int uuo_fit_set_joint_limits("):text.index("a weight per (frame, body joint)")]
    for word in ("[F][23]", "row j - 1", "F 207", "not sum w", "F = 1", "exact +0", "compact packing", "WORKSPACE",
                 "uuo_fit_set_foot_lock", "not copied", "Null switches the setting off", "w_pose == 0", "bit-reproducible",
                 "part stage", "w_soft", "lock-step", "-22", "unchanged"):
        assert word in note, word
