"""The heavy-tailed stress model (tests/stress_model.py) on the CPU: its statistics stay as stressful as the docstring
says, it survives the SMPL_NEUTRAL.pkl round trip and uuo_model_create's preconditions, and the float32 oracle's own
round-off against the float64 oracle on the stress inputs -- the level the GPU bounds of tests/test_gpu_model_range.py
refer to -- is measured and printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_model as sm  # noqa: E402

from uuo_mocap_amd.body_model import NUM_VERTS, synthetic_smpl  # noqa: E402

# The GPU forward bound is max(4 x this level, 1e-6 m), capped at 5e-6 m.  The level is about 1e-6 m and moves with the
# CPU's float32 matmul blocking (9.3e-7 and 1.2e-6 m seen on two machines); far above it the stress inputs have changed.
FP32_LEVEL_CAP = 2e-6


@pytest.fixture(scope="module")
def stress_tables(tmp_path_factory):
    return sm.load(sm.write_pkl(str(tmp_path_factory.mktemp("stress") / "SMPL_NEUTRAL.pkl")))


def test_generator_keeps_its_statistics(stress_tables):
    raw = sm.heavy_smpl(0)
    bscale = sm.skin16_scale(stress_tables)
    assert bscale == 1024.0  # the largest entry is 0.2 .. 0.25 m
    for name, basis in (("posedirs", stress_tables.posedirs), ("shapedirs", stress_tables.shapedirs)):
        a = np.abs(basis.astype(np.float64))
        nz = a[a > 0]
        # six decades, 1e-7 .. 1e-1 m, each holding at least 1 % of the non-zero entries (log-uniform, not a smooth basis)
        hist = np.histogram(np.log10(nz), bins=np.arange(-7.0, -0.5))[0]
        assert np.all(hist >= 0.01 * nz.size), (name, hist)
        assert nz.min() < 1e-9 and (a == 0).mean() > 0.1, name  # far below the hi plane's normal range, and exact zeros
        assert (a >= 0.1).sum() >= 10, name
        x = np.abs(basis.astype(np.float32)) * np.float32(bscale)
        assert ((x > 0) & (x < 2.0 ** -3)).sum() > 1000, name   # fp16 lo plane subnormal
        assert ((x > 0) & (x < 2.0 ** -14)).sum() > 1000, name  # hi plane subnormal too
    s0 = np.abs(stress_tables.shapedirs[..., 0])
    assert 0.18 <= s0.max() <= 0.25
    assert 0.1 <= np.abs(stress_tables.posedirs).max() <= 0.15
    # skin weights: <= 4 per vertex, most exactly 4, down to 1e-5, rows stochastic in float64 but not in float32
    W = stress_tables.lbs_weights
    nnz = (W != 0).sum(axis=1)
    assert nnz.max() == 4 and (nnz == 4).mean() > 0.85 and nnz.min() >= 2
    w = W[W > 0]
    assert w.min() <= 1e-5 and (w < 1e-4).mean() > 0.05 and (w < 1e-4).sum() > 1000
    assert (W >= 0).all()
    np.testing.assert_allclose(raw["weights"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (W.sum(axis=1, dtype=np.float32) != np.float32(1.0)).mean() > 0.05
    # joint regressor: non-negative, row-stochastic, 100 .. 300 non-zeros per row
    Jr = stress_tables.J_regressor
    rn = (Jr != 0).sum(axis=1)
    assert (Jr >= 0).all() and rn.min() >= 100 and rn.max() <= 300
    np.testing.assert_allclose(raw["J_regressor"].toarray().sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # deterministic
    again = sm.heavy_smpl.__wrapped__(0)
    for k in ("v_template", "shapedirs", "posedirs", "weights"):
        np.testing.assert_array_equal(again[k], raw[k], err_msg=k)


def test_model_survives_the_pickle_round_trip_and_model_create_preconditions(stress_tables):
    raw = sm.heavy_smpl(0)
    base = synthetic_smpl(0)
    V = NUM_VERTS
    t = stress_tables
    for k, v in (("v_template", raw["v_template"]), ("shapedirs", raw["shapedirs"]),
                 ("posedirs", raw["posedirs"].reshape(V * 3, -1).T), ("J_regressor", raw["J_regressor"].toarray()),
                 ("lbs_weights", raw["weights"])):
        got = getattr(t, k)
        assert got.dtype == np.float32, k
        np.testing.assert_array_equal(got, v.astype(np.float32), err_msg=k)
    assert t.posedirs.shape == (207, V * 3) and t.shapedirs.shape == (V, 3, 10) and t.J_regressor.shape == (24, V)
    np.testing.assert_array_equal(t.v_template, base.v_template)
    np.testing.assert_array_equal(t.faces, np.asarray(base.faces))
    assert t.faces.shape == (13776, 3)
    # uuo_model_create's preconditions (csrc/model.hip), checked here in Python
    assert ((t.lbs_weights != 0).sum(axis=1) <= 4).all()
    p = np.asarray(t.parents)
    assert p[0] == -1 and all(0 <= p[j] < j for j in range(1, 24))
    np.testing.assert_array_equal(p[1:], np.asarray(base.parents)[1:])
    ev = np.asarray(t.extra_joint_vids)
    assert ((ev >= 0) & (ev < V)).all()
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        assert np.isfinite(getattr(t, k)).all(), k


def test_stress_inputs_cover_the_folded_and_extreme_range():
    for F, seed in ((300, 0), (17, 1)):
        inp = sm.stress_inputs(F, seed)
        R = np.concatenate([inp["root"], inp["pose"]], axis=1).astype(np.float64)
        np.testing.assert_allclose(R @ np.swapaxes(R, -1, -2), np.broadcast_to(np.eye(3), R.shape), atol=1e-6)
        kind = inp["kind"]
        assert set(kind.tolist()) == {0, 1, 2}
        ang = np.arccos(np.clip((np.trace(R, axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0))
        assert (ang[kind == 0] < 1e-6).all()
        for j, _ in sm._FOLDS:  # folded joints at about pi - 0.3
            assert (np.abs(ang[kind == 1, j] - sm.FOLD) < 0.2).all(), j
        assert np.abs(inp["betas"]).max() > 4.0 and np.abs(inp["betas"]).max() <= 5.0
        assert np.abs(inp["betas_f"]).max() <= 5.0 and np.abs(inp["trans"]).max() <= 3.0


def test_fp32_oracle_level_on_the_stress_inputs(stress_tables, record_property):
    """The float32 oracle against the float64 oracle on the forward inputs of the GPU tests (per-frame betas in [-5, 5],
    folded and random poses, translations up to 3 m): the round-off level a correct float32 SMPL forward has here.
    tests/test_gpu_model_range.py recomputes it and bounds the kernels by 4 x this level."""
    for F, seed in ((300, 0), (17, 1)):
        ev, ej = sm.forward_error(stress_tables, sm.stress_inputs(F, seed))
        print("fp32 oracle vs float64 on the stress model, F=%d: vertices %.3e m, joints %.3e m" % (F, ev, ej))
        record_property("fp32_level_verts_F%d" % F, ev)
        record_property("fp32_level_joints_F%d" % F, ej)
        assert 0.0 < ev <= FP32_LEVEL_CAP and 0.0 < ej <= FP32_LEVEL_CAP, (F, ev, ej)
