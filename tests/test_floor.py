"""EXTENSION: the floor-contact term on sole vertices (stages.{chamfer,marker}.losses.floor_penetration / floor_contact) --
config validation and routing, the composed route's torch term against a numpy restatement, the default sole points, the floor
metric, the generator's floor and the C entry point's binding.  No GPU needed (tests/test_gpu_floor.py holds the fused closures
and the fits)."""
import os
import re
import subprocess
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(name="video_mocap", **stages):
    """packaged config; per stage a dict whose `floor_height` / `floor_points` entries go on the stage, the rest on its losses"""
    from uuo_mocap_amd.config import packaged_config

    cfg = packaged_config(name)
    for stage, kv in stages.items():
        for k, v in kv.items():
            if k in ("floor_height", "floor_points"):
                cfg["stages"][stage][k] = v
            else:
                cfg["stages"][stage]["losses"][k] = v
    return cfg


# ------------------------------------------------------------------------------------------------ 1. config, refusals, routing
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_floor_keys_are_read_and_validated(stage):
    from uuo_mocap_amd.engine import stage_floor

    assert stage_floor(_cfg(), stage) == {"w_pen": 0.0, "w_con": 0.0, "height": 0.0, "points": None}   # absent: off
    assert stage_floor(_cfg(**{stage: {"floor_penetration": None, "floor_contact": 0}}), stage)["w_pen"] == 0.0
    fl = stage_floor(_cfg(**{stage: {"floor_penetration": 2.5, "floor_contact": 4.0, "floor_height": -0.25,
                                     "floor_points": [[3, 1], [7]]}}), stage)
    assert fl == {"w_pen": 2.5, "w_con": 4.0, "height": -0.25, "points": [[3, 1], [7]]}
    for key in ("floor_penetration", "floor_contact"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=key):
                stage_floor(_cfg(**{stage: {key: bad}}), stage)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="floor_height"):
            stage_floor(_cfg(**{stage: {"floor_height": bad}}), stage)
    for bad in ([[1, 2]], [[1], []], [[], [2]], [[1], [2.5]], [[-1], [2]], [1, 2], "soles", [list(range(9)), list(range(8))],
                [[True], [2]]):
        with pytest.raises(ValueError, match="floor_points"):
            stage_floor(_cfg(**{stage: {"floor_points": bad}}), stage)
    assert len(sum(stage_floor(_cfg(**{stage: {"floor_points": [list(range(8)), list(range(8))]}}), stage)["points"], [])) == 16


def test_stage_problems_refuse_bad_keys_before_touching_the_device():
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem

    with pytest.raises(ValueError, match="floor_penetration"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"floor_penetration": -2.0}))
    with pytest.raises(ValueError, match="floor_contact"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"floor_contact": float("nan")}))
    with pytest.raises(NotImplementedError, match="soft"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"floor_penetration": 1.0, "soft_chamfer": 10.0}))
    with pytest.raises(NotImplementedError, match="floor_penetration"):
        PartProblem(None, None, None, None, None, None, _cfg(part={"floor_penetration": 1.0}))
    with pytest.raises(NotImplementedError, match="floor_contact"):
        PartProblem(None, None, None, None, None, None, _cfg(part={"floor_contact": 1.0}))
    with pytest.raises(NotImplementedError, match="tracklets.*floor"):
        MarkerProblem(None, torch.zeros(3, 2, 3), None, None, None, _cfg(marker={"floor_penetration": 1.0}),
                      frame_assign=torch.zeros(3, 2, dtype=torch.int32))


def test_routing_flags():
    from uuo_mocap_amd.optimization import lockstep_supported
    from uuo_mocap_amd.terms import FLOOR, StageTerms

    _floor_on = lambda cfg, stage: StageTerms(cfg, stage).on(FLOOR)
    _floor_fused = lambda cfg, stage: StageTerms(cfg, stage).fused(FLOOR)

    plain, floor = _cfg(), _cfg("video_mocap_floor")
    for stage in ("chamfer", "marker"):
        assert not _floor_on(plain, stage) and _floor_on(floor, stage)
        assert lockstep_supported(_cfg(**{stage: {"floor_penetration": 0.0, "floor_contact": 0.0}}), stage)
        assert not lockstep_supported(floor, stage)          # lock-step batches do not carry the term
        assert not lockstep_supported(_cfg(**{stage: {"floor_penetration": 1.0}}), stage)
        assert not lockstep_supported(_cfg(**{stage: {"floor_contact": 1.0}}), stage)
        assert _floor_fused(floor, stage)
        composed = _cfg("video_mocap_floor")
        composed["execution"] = {"floor_fused": False}
        assert not _floor_fused(composed, stage)
        assert _floor_fused(dict(plain, execution={"floor_fused": False}), stage)  # nothing to compose without the term


def _zeros(*s):
    return torch.zeros(*s)


class _Smpl:
    class device_model:
        V = 6890


def test_composed_routes_are_taken(monkeypatch):
    """execution.floor_fused: False and soft_chamfer + floor go to the closures composed from the operators"""
    from uuo_mocap_amd import optimization as opt

    F, M = 6, 4
    markers = _zeros(F, M, 3)
    one_hot = _zeros(M, 6890)
    one_hot[:, 0] = 1.0
    taken = []

    def chamfer_general(*a, **k):
        taken.append("chamfer")

    def markers_general(*a, **k):
        taken.append("marker")

    monkeypatch.setattr(opt, "_optim_chamfer_general", chamfer_general)
    monkeypatch.setattr(opt, "_optim_markers_general", markers_general)
    cfg = _cfg("video_mocap_floor")
    cfg["execution"] = {"floor_fused": False}
    args_c = (markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3), _zeros(F, 3),
              _zeros(F), torch.zeros(F, M, dtype=torch.long), None)
    opt.optim_chamfer(*args_c, cfg)
    opt.optim_markers(markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3),
                      _zeros(F, 3), one_hot, _zeros(F), _Smpl, cfg)
    assert taken == ["chamfer", "marker"]
    soft = _cfg("video_mocap_floor", chamfer={"soft_chamfer": 10.0})
    opt.optim_chamfer(*args_c, soft)   # (markers on the host: the fused soft closure is not in reach either way)
    assert taken == ["chamfer", "marker", "chamfer"]


def test_frame_sharding_refuses_the_term():
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.optimization import optim_chamfer, optim_markers

    F, M = 6, 4
    markers = _zeros(F, M, 3)
    one_hot = _zeros(M, 6890)
    one_hot[:, 0] = 1.0
    for keys in ({"floor_penetration": 1.0}, {"floor_contact": 1.0}):
        with parallel.shard_frames(joint_with_one_rank=True):
            with pytest.raises(NotImplementedError, match="floor_penetration / floor_contact.*frame-block sharding"):
                optim_chamfer(markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3),
                              _zeros(F, 3), _zeros(F), torch.zeros(F, M, dtype=torch.long), None, _cfg(chamfer=keys),
                              foot_contacts=torch.ones(F, 2))
            with pytest.raises(NotImplementedError, match="floor_penetration / floor_contact.*frame-block sharding"):
                optim_markers(markers, _zeros(F, 23, 3, 3), _zeros(F, 23, 3, 3), _zeros(1, 10), _zeros(1, 10), _zeros(F, 1, 3, 3),
                              _zeros(F, 3), one_hot, _zeros(F), _Smpl, _cfg(marker=keys), foot_contacts=torch.ones(F, 2))


def test_solve_batch_refuses_the_term_up_front():
    from uuo_mocap_amd.engine import solve_batch

    class _P:
        model = None
        joint_accel = 0.0
        foot_lock = 0.0
        floor_on = True

        class problem:
            w_offsets = 0.0

    with pytest.raises(NotImplementedError, match="floor_penetration / floor_contact"):
        solve_batch([_P()], [None], max_iter=1)


def test_shipped_floor_config_differs_from_its_parent_only_by_the_term():
    from uuo_mocap_amd.engine import stage_floor

    plain, floor = _cfg(), _cfg("video_mocap_floor")
    new_losses, new_keys = ("floor_penetration", "floor_contact"), ("losses", "floor_height", "floor_points")
    for stage in ("chamfer", "marker"):
        fl = stage_floor(floor, stage)
        assert fl["w_pen"] > 0.0 and fl["w_con"] > 0.0 and fl["height"] == 0.0 and fl["points"] is None
        rest = {k: v for k, v in floor["stages"][stage]["losses"].items() if k not in new_losses}
        assert rest == plain["stages"][stage]["losses"]
        assert {k: v for k, v in floor["stages"][stage].items() if k not in new_keys} == \
            {k: v for k, v in plain["stages"][stage].items() if k != "losses"}
    for stage in plain["stages"]:
        if stage not in ("chamfer", "marker"):
            assert floor["stages"][stage] == plain["stages"][stage]
    strip = lambda c: {k: v for k, v in c.items() if k not in ("stages", "name", "parent")}
    assert strip(floor) == strip(plain)


# ------------------------------------------------------------------------------------------------ 2. the composed term
def _np_floor(z, k_left, c, h, w_pen, w_con):
    """numpy float64 restatement of the issue's formula on sole heights z [F, K]: the value and d / dz [F, K]"""
    F, K = z.shape
    g = np.zeros_like(z)
    total = 0.0
    for t in range(F):
        for p in range(K):
            pen = max(h - z[t, p], 0.0)
            total += w_pen * pen * pen / (F * K)
            g[t, p] += -2.0 * w_pen * pen / (F * K)
        for s, (lo, hi) in enumerate(((0, k_left), (k_left, K))):
            am = lo
            for p in range(lo + 1, hi):
                if z[t, p] < z[t, am]:  # strict: the first in list order keeps an exact tie
                    am = p
            flo = max(z[t, am] - h, 0.0)
            if c is not None:
                total += w_con * c[t, s] * flo * flo / (2.0 * F)
                g[t, am] += w_con * c[t, s] * flo / F
    return total, g


@pytest.mark.parametrize("F,K,k_left", [(1, 2, 1), (3, 6, 3), (8, 16, 5), (5, 7, 6)])
def test_composed_term_matches_a_numpy_restatement(F, K, k_left):
    from uuo_mocap_amd.losses import floor_loss

    rng = np.random.default_rng(70 + F)
    V = 40
    verts = rng.normal(size=(F, V, 3)) * 0.05
    vids = rng.permutation(V)[:K]
    c = rng.uniform(size=(F, 2))
    c[0, 0] = 0.0
    c[-1, 1] = 1.0
    h, w_pen, w_con = 0.01, 3.0, 7.0
    vt = torch.tensor(verts, requires_grad=True)
    loss = floor_loss(vt, vids, k_left, torch.tensor(c), h, w_pen, w_con)
    loss.backward()
    lo, gz = _np_floor(verts[:, vids, 2], k_left, c, h, w_pen, w_con)
    assert lo > 0.0 and np.abs(gz).max() > 0.0
    assert float(loss) == pytest.approx(lo, rel=1e-12, abs=0.0)
    g = np.zeros_like(verts)
    g[:, vids, 2] = gz
    np.testing.assert_allclose(vt.grad.numpy(), g, rtol=1e-10, atol=1e-15)
    assert not vt.grad[..., :2].any()                                   # x and y: exact zeros
    # the penetration piece alone needs no labels; contacts None or weight 0 drop the contact piece
    for contacts, wc in ((None, w_con), (torch.tensor(c), 0.0)):
        lp = floor_loss(torch.tensor(verts), vids, k_left, contacts, h, w_pen, wc)
        assert float(lp) == pytest.approx(_np_floor(verts[:, vids, 2], k_left, None, h, w_pen, 0.0)[0], rel=1e-12)


def test_composed_term_exact_tie_goes_to_the_first_in_list_order():
    from uuo_mocap_amd.losses import floor_loss

    F, V = 2, 10
    verts = np.zeros((F, V, 3))
    verts[..., 2] = np.linspace(0.05, 0.09, V)[None]
    vids = [7, 2, 5, 4, 9, 1]          # left: 7, 2, 5   right: 4, 9, 1
    verts[:, 2, 2] = 0.03              # an exact tie of the left foot's two lowest points, list positions 1 and 2
    verts[:, 5, 2] = 0.03
    verts[1, 9, 2] = 0.02              # frame 1, right foot: an exact tie of list positions 1 and 2 again
    verts[1, 1, 2] = 0.02
    c = np.ones((F, 2))
    vt = torch.tensor(verts, requires_grad=True)
    loss = floor_loss(vt, vids, 3, torch.tensor(c), 0.0, 0.0, 1.0)
    loss.backward()
    lo, gz = _np_floor(verts[:, vids, 2], 3, c, 0.0, 0.0, 1.0)
    assert float(loss) == pytest.approx(lo, rel=1e-12)
    g = vt.grad.numpy()[..., 2]
    assert g[0, 2] == pytest.approx(0.03 / F) and g[0, 5] == 0.0        # vertex 2 (first in the list) takes all of it
    assert g[1, 9] == pytest.approx(0.02 / F) and g[1, 1] == 0.0
    np.testing.assert_allclose(g[:, vids], gz, rtol=1e-12, atol=0.0)


def test_composed_term_exact_zeros():
    from uuo_mocap_amd.losses import floor_loss

    F, V = 4, 12
    verts = torch.rand(F, V, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(7)) + 0.1   # all in [0.1, 1.1)
    vids = [0, 1, 2, 3]
    assert float(floor_loss(verts, vids, 2, torch.zeros(F, 2), 0.0, 5.0, 5.0)) == 0.0   # no penetration, no contact
    assert float(floor_loss(verts, vids, 2, None, 0.0, 5.0, 5.0)) == 0.0
    assert float(floor_loss(verts, vids, 2, torch.ones(F, 2), 0.0, 5.0, 0.0)) == 0.0
    assert float(floor_loss(verts, vids, 2, torch.ones(F, 2), 0.0, 0.0, 5.0)) > 0.0      # hovering in contact
    assert float(floor_loss(verts - 2.0, vids, 2, torch.ones(F, 2), 0.0, 0.0, 5.0)) == 0.0  # all below: the contact piece is silent
    assert floor_loss(verts.float(), vids, 2, torch.ones(F, 2, dtype=torch.float64), 0.0, 1.0, 1.0).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. default sole points
def test_sole_vertices(tables):
    from uuo_mocap_amd.body_model import sole_vertices

    owner = np.argmax(tables.lbs_weights, axis=1)
    vt = tables.v_template.astype(np.float64)
    for per_foot in (1, 3, 8):
        sv = sole_vertices(tables, per_foot=per_foot)
        assert sv.shape == (2, per_foot) and sv.dtype == np.int64
        assert np.array_equal(sv, sole_vertices(tables, per_foot=per_foot))          # deterministic
        assert len(set(sv.reshape(-1).tolist())) == 2 * per_foot                      # distinct ids
        for s in range(2):
            assert (owner[sv[s]] == 10 + s).all()                                     # owned by the foot joint
            foot = np.where(owner == 10 + s)[0]
            assert (vt[sv[s], 1] <= vt[foot, 1].min() + 0.010 + 1e-12).all()          # within the 10 mm band of the sole
            assert vt[sv[s, 0], 1] == vt[foot, 1].min()                               # started at the lowest
    assert np.array_equal(sole_vertices(tables), sole_vertices(tables, per_foot=3))
    for s in range(2):                                                                # the band holds 14 and 12 candidates
        foot = np.where(owner == 10 + s)[0]
        assert int((vt[foot, 1] <= vt[foot, 1].min() + 0.010).sum()) == (14, 12)[s]
    with pytest.raises(ValueError):
        sole_vertices(tables, per_foot=15)
    with pytest.raises(ValueError):
        sole_vertices(tables, per_foot=0)
    # the smplx heel and toe picks are NOT at the feet of the synthetic model: the reason the default is geometric
    assert not np.isin(owner[tables.extra_joint_vids[5:11]], [10, 11]).any()


# ------------------------------------------------------------------------------------------------ 4. metric
def test_floor_error_known_answers():
    from uuo_mocap_amd.metrics import compute_floor_error

    z = torch.tensor([[0.010, 0.020, -0.004, 0.030],     # left low 10 mm, right 4 mm under
                      [0.000, 0.005, 0.006, 0.002],      # left on the floor, right 2 mm over
                      [-0.002, -0.006, 0.050, 0.040]])   # left 6 mm under, right 40 mm over
    c = torch.tensor([[1.0, 1.0], [0.0, 1.0], [1.0, 0.5]])
    e = compute_floor_error(z, 2, c, 0.0)
    assert e["penetration_mm"] == pytest.approx((4.0 + 2.0 + 6.0) / 12.0, rel=1e-6)
    assert e["max_penetration_mm"] == pytest.approx(6.0, rel=1e-6)
    assert e["float_mm"] == pytest.approx((10.0 + 0.0 + 2.0 + 0.0) / 4.0, rel=1e-6)   # (0, L) (0, R) (1, R) (2, L); 0.5 is no contact
    e = compute_floor_error(z, 2, torch.zeros(3, 2), 0.0)
    assert e["float_mm"] == 0.0 and e["penetration_mm"] > 0.0                          # the empty case: 0.0, not NaN
    e = compute_floor_error(z + 0.1, 2, c, 0.1)                                        # the plane's height shifts with the body
    assert e["max_penetration_mm"] == pytest.approx(6.0, rel=1e-5)
    e = compute_floor_error(z, 3, c, 0.0)                                              # the split between the feet matters
    assert e["float_mm"] == pytest.approx((0.0 + 30.0 + 2.0 + 0.0) / 4.0, rel=1e-6)
    for bad in (lambda: compute_floor_error(z, 0, c, 0.0), lambda: compute_floor_error(z, 4, c, 0.0),
                lambda: compute_floor_error(z, 2, c[:2], 0.0), lambda: compute_floor_error(z[0], 2, c, 0.0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ 5. generator
@pytest.fixture(scope="module")
def floor_sequences(tables):
    from uuo_mocap_amd.synthetic import make_sequence

    F, M = 90, 12
    return (make_sequence(tables, seed=0, num_frames=F, num_markers=M, planted_feet=True),
            make_sequence(tables, seed=0, num_frames=F, num_markers=M, planted_feet=True, floor=False),
            make_sequence(tables, seed=0, num_frames=F, num_markers=M, planted_feet=True, floor=True))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_floor_option_off_changes_nothing(floor_sequences):
    base, off, _ = floor_sequences
    assert set(base.gt) == set(off.gt) and not {"sole_vids", "floor_height", "sole_z"} & set(base.gt)
    for k in base.gt:
        assert _same(base.gt[k], off.gt[k]), k
    for k, v in vars(base.img_smpl).items():
        assert _same(v, getattr(off.img_smpl, k)), k
    assert np.array_equal(base.markers.get_points(), off.markers.get_points())


def test_floor_sequence(tables, floor_sequences):
    from uuo_mocap_amd.body_model import sole_vertices
    from uuo_mocap_amd.synthetic import lbs_f64, make_sequence

    base, _, seq = floor_sequences
    F = 90
    assert np.array_equal(seq.gt["sole_vids"], sole_vertices(tables)) and seq.gt["floor_height"] == 0.0
    z = seq.gt["sole_z"]
    assert z.dtype == np.float64 and z.shape == (F, 6)
    assert np.abs(z.min(axis=1)).max() <= 1e-9 and z.min() >= 0.0        # the lowest sole point ON the floor, none below
    # ... and that is the body the capture holds: the float32 ground truth reproduces the heights to float32 accuracy
    v, _, _ = lbs_f64(tables, seq.gt["rot"].astype(np.float64), seq.gt["betas"].astype(np.float64), seq.gt["trans"].astype(np.float64))
    assert np.abs(v[:, seq.gt["sole_vids"].reshape(-1), 2] - z).max() <= 2e-6
    assert np.abs(seq.gt["verts"][:, seq.gt["sole_vids"].reshape(-1), 2] - z).max() <= 2e-6
    # x and y of the planted translation are kept; the pose track, shape and marker vertices too
    assert np.array_equal(seq.gt["trans"][:, :2], base.gt["trans"][:, :2])
    assert np.array_equal(seq.gt["rot"], base.gt["rot"]) and np.array_equal(seq.gt["betas"], base.gt["betas"])
    assert np.array_equal(seq.gt["marker_vids"], base.gt["marker_vids"])
    assert torch.equal(seq.img_smpl.pose_body, base.img_smpl.pose_body)
    # labels only where they are defined: the stance foot, its lowest sole point within 5 mm of the floor
    c, stance = seq.gt["foot_contacts"], base.gt["foot_contacts"]
    low = np.stack([z[:, :3].min(axis=1), z[:, 3:].min(axis=1)], axis=1)
    assert set(np.unique(c)) <= {0.0, 1.0} and c.sum() > 0
    assert np.array_equal(c == 1.0, (stance == 1.0) & (low <= 0.005))
    seen = seq.img_smpl.foot_contacts.numpy()
    assert (seen <= c).all() and 0 < seen.sum() < c.sum()                 # eroded labels: a subset, never wrong
    for s in range(2):                                                    # two frames off each end of every run
        on = np.concatenate([[0.0], c[:, s], [0.0]])
        for a0, b0 in zip(np.where(np.diff(on) > 0)[0], np.where(np.diff(on) < 0)[0]):
            expect = np.zeros(b0 - a0)
            expect[2:max(b0 - a0 - 2, 2)] = 1.0
            assert np.array_equal(seen[a0:b0, s], expect)
    with pytest.raises(ValueError, match="planted_feet"):
        make_sequence(tables, seed=0, num_frames=8, num_markers=8, floor=True)


# ------------------------------------------------------------------------------------------------ 6. C entry point
def test_entry_point_is_declared_bound_and_typed_as_in_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    assert "uuo_fit_set_floor" in _lib.header_symbols()
    sig = [c_void_p, c_float, c_float, c_float, c_void_p, c_int, c_int, c_void_p]
    assert _lib._SIGNATURES["uuo_fit_set_floor"] == (c_int, sig)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+uuo_fit_set_floor\s*\(\s*uuo_fit_t\s*\*\s*fit\s*,\s*float\s+w_pen\s*,\s*float\s+w_con\s*,\s*float\s+"
                     r"height\s*,\s*const\s+int32_t\s*\*\s*d_vids\s*,\s*int32_t\s+k_left\s*,\s*int32_t\s+k_right\s*,\s*const\s+float"
                     r"\s*\*\s*d_contacts\s*\)\s*;", text)
    src = tmp_path / "sig.c"
    src.write_text('#include "uuo_hip.h"\nint (*fp)(uuo_fit_t*, float, float, float, const int32_t*, int32_t, int32_t, const float*) '
                   '= uuo_fit_set_floor;\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "sig.o")])
    assert _lib.ABI_VERSION == 3  # the problem structure and the ABI version did not change
    lib = _lib.load()             # (dlopen needs no GPU) bound with the declared types
    assert lib.uuo_fit_set_floor.argtypes == sig and lib.uuo_fit_set_floor.restype == c_int


def test_note_in_the_header():
    from uuo_mocap_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    note = text[text.index("floor-contact term on K"):text.index("int uuo_fit_set_floor")]
    for word in ("z is up", "m^2", "first in list order", "d_vids", "d_contacts", "2 .. 16", "F = 1", "part stage", "lock-step"):
        assert word in note, word
