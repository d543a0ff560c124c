"""EXTENSION: the contact-gated foot-lock term (stages.{chamfer,marker}.losses.foot_lock) -- config validation and routing, the
composed route's torch term against a numpy restatement, the foot-skate metric, the planted-feet generator and the C entry
point's binding.  No GPU needed (tests/test_gpu_foot_lock.py holds the fused closures and the fits)."""
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


# ------------------------------------------------------------------------------------------------ 1. config, refusals, routing
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_foot_lock_is_read_and_validated(stage):
    from uuo_mocap_amd.engine import stage_foot_lock

    assert stage_foot_lock(_cfg(), stage) == 0.0                                     # absent: off
    assert stage_foot_lock(_cfg(**{stage: {"foot_lock": 0}}), stage) == 0.0
    assert stage_foot_lock(_cfg(**{stage: {"foot_lock": None}}), stage) == 0.0
    assert stage_foot_lock(_cfg(**{stage: {"foot_lock": 2.5}}), stage) == pytest.approx(2.5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="foot_lock"):
            stage_foot_lock(_cfg(**{stage: {"foot_lock": bad}}), stage)


def test_stage_problems_refuse_bad_weights_and_contacts_before_touching_the_device():
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, check_foot_contacts

    with pytest.raises(ValueError, match="foot_lock"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"foot_lock": -2.0}))
    with pytest.raises(ValueError, match="foot_lock"):
        MarkerProblem(None, None, None, None, None, _cfg(marker={"foot_lock": float("nan")}))
    with pytest.raises(NotImplementedError, match="soft"):
        ChamferProblem(None, None, None, None, None, _cfg(chamfer={"foot_lock": 1.0, "soft_chamfer": 10.0}))
    # contact arrays: shape, finiteness, range -- (smpl_inference is None: anything that went further would fail differently)
    F = 5
    markers = torch.zeros(F, 4, 3)
    good = torch.rand(F, 2)
    bads = {"frames": torch.rand(F + 1, 2), "feet": torch.rand(F, 3), "rank": torch.rand(F), "nan": good.clone(),
            "inf": good.clone(), "negative": good.clone(), "above one": good.clone()}
    bads["nan"][2, 0] = float("nan")
    bads["inf"][1, 1] = float("inf")
    bads["negative"][0, 0] = -1e-3
    bads["above one"][4, 1] = 1.001
    for on in (1.0, 0.0):  # the labels are checked whether or not the key is on
        for tag, bad in bads.items():
            with pytest.raises(ValueError, match="foot_contacts"):
                ChamferProblem(None, markers, None, None, None, _cfg(chamfer={"foot_lock": on}), foot_contacts=bad)
            with pytest.raises(ValueError, match="foot_contacts"):
                MarkerProblem(None, markers, None, None, None, _cfg(marker={"foot_lock": on}), foot_contacts=bad.numpy())
    assert check_foot_contacts(None, F) is None
    c = check_foot_contacts(good.double().numpy(), F)
    assert c.dtype == torch.float32 and tuple(c.shape) == (F, 2) and c.device.type == "cpu"
    assert check_foot_contacts(torch.tensor([[0.0, 1.0]]), 1) is not None  # the closed range


def test_foot_lock_in_the_part_stage_is_refused():
    from uuo_mocap_amd.engine import PartProblem

    with pytest.raises(NotImplementedError, match="foot_lock"):
        PartProblem(None, None, None, None, None, None, _cfg(part={"foot_lock": 1.0}))


def test_routing_flags():
    from uuo_mocap_amd.optimization import lockstep_supported
    from uuo_mocap_amd.terms import FOOT_LOCK, JOINT_ACCEL, StageTerms

    _temporal_fused = lambda cfg, stage: all(StageTerms(cfg, stage).fused(t) for t in (JOINT_ACCEL, FOOT_LOCK))  # one switch for both

    plain, contact = _cfg(), _cfg("video_mocap_contact")
    for stage in ("chamfer", "marker"):
        assert lockstep_supported(_cfg(**{stage: {"foot_lock": 0.0}}), stage)
        assert not lockstep_supported(contact, stage)          # lock-step batches do not carry the term
        assert not lockstep_supported(_cfg(**{stage: {"foot_lock": 1.0}}), stage)
        assert _temporal_fused(contact, stage)
        contact_c = _cfg("video_mocap_contact")
        contact_c["execution"] = {"temporal_fused": False}
        assert not _temporal_fused(contact_c, stage)
        assert _temporal_fused(dict(plain, execution={"temporal_fused": False}), stage)  # nothing to compose without a term


def test_frame_sharding_refuses_the_term():
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.optimization import optim_chamfer, optim_markers

    F, M = 6, 4
    markers = torch.zeros(F, M, 3)
    z = lambda *s: torch.zeros(*s)
    one_hot = torch.zeros(M, 6890)
    one_hot[:, 0] = 1.0

    class _Smpl:
        class device_model:
            V = 6890

    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="foot_lock.*frame-block sharding"):
            optim_chamfer(markers, z(F, 23, 3, 3), z(F, 23, 3, 3), z(1, 10), z(1, 10), z(F, 1, 3, 3), z(F, 3), z(F),
                          torch.zeros(F, M, dtype=torch.long), None, _cfg("video_mocap_contact"), foot_contacts=torch.ones(F, 2))
        with pytest.raises(NotImplementedError, match="foot_lock.*frame-block sharding"):
            optim_markers(markers, z(F, 23, 3, 3), z(F, 23, 3, 3), z(1, 10), z(1, 10), z(F, 1, 3, 3), z(F, 3), one_hot, z(F),
                          _Smpl, _cfg("video_mocap_contact"), foot_contacts=torch.ones(F, 2))


def test_solve_batch_refuses_the_term_up_front():
    from uuo_mocap_amd.engine import solve_batch

    class _P:
        model = None
        joint_accel = 0.0
        foot_lock = 3.0

        class problem:
            w_offsets = 0.0

    with pytest.raises(NotImplementedError, match="foot-lock"):
        solve_batch([_P()], [None], max_iter=1)


def test_shipped_contact_config_differs_from_its_parent_only_by_the_term():
    from uuo_mocap_amd.engine import stage_foot_lock

    plain, contact = _cfg(), _cfg("video_mocap_contact")
    assert stage_foot_lock(contact, "chamfer") > 0.0 and stage_foot_lock(contact, "marker") > 0.0
    assert "foot_lock" not in contact["stages"]["part"]["losses"]
    for stage in ("chamfer", "marker"):
        rest = {k: v for k, v in contact["stages"][stage]["losses"].items() if k != "foot_lock"}
        assert rest == plain["stages"][stage]["losses"]
        assert {k: v for k, v in contact["stages"][stage].items() if k != "losses"} == \
            {k: v for k, v in plain["stages"][stage].items() if k != "losses"}
    for stage in plain["stages"]:
        if stage not in ("chamfer", "marker"):
            assert contact["stages"][stage] == plain["stages"][stage]
    strip = lambda c: {k: v for k, v in c.items() if k not in ("stages", "name", "parent")}
    assert strip(contact) == strip(plain)


# ------------------------------------------------------------------------------------------------ 2. the composed term
def _np_lock(j, c):
    """numpy float64 restatement of the issue's formula: feet = joints 10, 11; g[t, s] = c[t, s] c[t-1, s];
    v[t, s] = J[t, foot_s] - J[t-1, foot_s], t = 1 .. F-1; term = sum g |v|^2 / ((F - 1) 6);
    d/dJ[f, foot_s] = (2 / ((F - 1) 6)) (g[f, s] v[f, s] - g[f+1, s] v[f+1, s]), terms outside 1 .. F-1 dropped."""
    F = j.shape[0]
    g = np.zeros_like(j)
    if F < 2:
        return 0.0, g
    n = (F - 1) * 6.0
    total = 0.0
    for s, foot in enumerate((10, 11)):
        for t in range(1, F):
            gate = c[t, s] * c[t - 1, s]
            v = j[t, foot] - j[t - 1, foot]
            total += gate * float(v @ v)
            g[t, foot] += 2.0 * gate * v / n
            g[t - 1, foot] -= 2.0 * gate * v / n
    return total / n, g


@pytest.mark.parametrize("F", [1, 2, 3, 8])
def test_composed_term_matches_a_numpy_restatement(F):
    from uuo_mocap_amd.losses import foot_lock_loss

    rng = np.random.default_rng(40 + F)
    j = rng.normal(size=(F, 24, 3)) * 0.3 + np.arange(F)[:, None, None] * 0.01
    c = rng.uniform(size=(F, 2))
    jt = torch.tensor(j, requires_grad=True)
    loss = foot_lock_loss(jt, torch.tensor(c))
    loss.backward()
    lo, g = _np_lock(j, c)
    if F == 1:
        assert float(loss) == 0.0 and not jt.grad.any()
    else:
        assert lo > 0.0
        assert float(loss) == pytest.approx(lo, rel=1e-12, abs=0.0)
        np.testing.assert_allclose(jt.grad.numpy(), g, rtol=1e-10, atol=1e-15)
        other = [k for k in range(24) if k not in (10, 11)]
        assert not jt.grad[:, other].any()  # the feet only


def test_composed_term_exact_zeros_and_closed_form():
    from uuo_mocap_amd.losses import foot_lock_loss

    F = 9
    j = torch.randn(F, 24, 3, dtype=torch.float64)
    assert float(foot_lock_loss(j, torch.zeros(F, 2, dtype=torch.float64))) == 0.0   # no contacts
    one = torch.zeros(F, 2, dtype=torch.float64)
    one[4, 0] = 1.0
    one[7, 1] = 1.0
    assert float(foot_lock_loss(j, one)) == 0.0                                      # a one-frame contact: the gate is a product
    still = j.clone()
    still[:, 10:12] = still[0:1, 10:12]                                              # rigidly still feet, everything else moving
    assert float(foot_lock_loss(still, torch.ones(F, 2, dtype=torch.float64))) == 0.0
    # a foot at constant velocity u under full contact, the other still: sum = (F - 1) |u|^2 over (F - 1) 6 entries
    u = torch.tensor([0.01, -0.02, 0.005], dtype=torch.float64)
    walk = still.clone()
    walk[:, 10] = still[0, 10] + torch.arange(F, dtype=torch.float64)[:, None] * u
    assert float(foot_lock_loss(walk, torch.ones(F, 2, dtype=torch.float64))) == pytest.approx(float(u @ u) / 6.0, rel=1e-12)
    # float32 joints with float64 or float32 labels, and labels on the joints' device and dtype
    assert foot_lock_loss(walk.float(), torch.ones(F, 2, dtype=torch.float64)).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. metric
def test_foot_skate_known_answers():
    from uuo_mocap_amd.metrics import compute_foot_skate

    F, freq = 10, 30.0
    j = torch.zeros(F, 24, 3, dtype=torch.float64)
    j[:, 10, 0] = torch.arange(F, dtype=torch.float64) * 0.003       # left foot slides 3 mm a frame
    j[:, 11, 2] = torch.arange(F, dtype=torch.float64) ** 2 * 0.001  # right foot accelerates
    j[:, 5] = torch.randn(F, 3, dtype=torch.float64)                 # another joint: ignored
    c = torch.zeros(F, 2)
    assert float(compute_foot_skate(j, c, freq)) == 0.0              # the empty case: 0.0, not NaN
    c[:, 0] = 1.0
    assert float(compute_foot_skate(j, c, freq)) == pytest.approx(0.003 * freq, rel=1e-12)
    c[:] = 0.0
    c[3:6, 1] = 1.0                                                   # pairs (4, 3) and (5, 4) of the right foot
    expect = ((16 - 9) + (25 - 16)) / 2 * 0.001 * freq
    assert float(compute_foot_skate(j, c, freq)) == pytest.approx(expect, rel=1e-12)
    c[4, 1] = 0.5                                                     # fractional labels do not count as contact
    assert float(compute_foot_skate(j, c, freq)) == 0.0
    c[:] = 0.0
    c[2, 0] = 1.0                                                     # a single frame has no pair
    assert float(compute_foot_skate(j, c, freq)) == 0.0
    assert float(compute_foot_skate(j[:1], torch.ones(1, 2), freq)) == 0.0
    assert float(compute_foot_skate(torch.zeros(F, 45, 3), torch.ones(F, 2), freq)) == 0.0
    with pytest.raises(ValueError):
        compute_foot_skate(j, torch.ones(F + 1, 2), freq)
    with pytest.raises(ValueError):
        compute_foot_skate(j[:, :12], torch.ones(F, 2), freq)


# ------------------------------------------------------------------------------------------------ 4. generator
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_feet_sequence(tables, seed):
    from uuo_mocap_amd.synthetic import make_sequence

    F = 300
    base = make_sequence(tables, seed=seed, num_frames=F, num_markers=50)
    seq = make_sequence(tables, seed=seed, num_frames=F, num_markers=50, planted_feet=True)
    c = seq.gt["foot_contacts"]
    assert c.shape == (F, 2) and set(np.unique(c)) == {0.0, 1.0}
    assert (c.sum(axis=1) == 1.0).all()                               # one stance foot per frame
    assert (c[:20, 0] == 1.0).all() and (c[20:40, 1] == 1.0).all()    # stance_frames = 20, left first
    j = seq.gt["joints"].astype(np.float64)
    step = np.linalg.norm(j[1:, 10:12] - j[:-1, 10:12], axis=-1)      # [F-1, 2]
    gate = c[1:] * c[:-1]
    assert gate.sum() == 285
    assert step[gate == 1.0].max() <= 1e-6                            # the contact foot does not move (float32 storage)
    assert step[gate == 0.0].mean() > 5e-3                            # the swing foot does
    seen = seq.img_smpl.foot_contacts.numpy()
    assert seen.shape == (F, 2) and set(np.unique(seen)) == {0.0, 1.0}
    assert (seen <= c).all() and seen.sum() < c.sum()                 # eroded labels: a subset, never wrong
    for a0 in range(0, F, 20):                                        # two frames off each end of every stance
        s = int(c[a0, 1])
        assert not seen[a0:a0 + 2, s].any() and not seen[a0 + 18:a0 + 20, s].any() and seen[a0 + 2:a0 + 18, s].all()
    assert np.ptp(seq.gt["trans"], axis=0).max() <= 1.5
    # the pose track (ground truth and HMR stand-in) is the default call's; the first frame's translation too
    assert np.array_equal(seq.gt["rot"], base.gt["rot"]) and np.array_equal(seq.gt["betas"], base.gt["betas"])
    assert torch.equal(seq.img_smpl.pose_body, base.img_smpl.pose_body)
    assert torch.equal(seq.img_smpl.root_orient, base.img_smpl.root_orient)
    assert np.array_equal(seq.gt["trans"][0], base.gt["trans"][0])
    assert np.array_equal(seq.gt["marker_vids"], base.gt["marker_vids"])
    # a default call is what it was: no labels, no new key
    assert not base.img_smpl.foot_contacts.any() and "foot_contacts" not in base.gt


def test_planted_feet_stance_length_and_short_sequences(tables):
    from uuo_mocap_amd.synthetic import make_sequence

    seq = make_sequence(tables, seed=1, num_frames=23, num_markers=8, planted_feet=True, stance_frames=5)
    c = seq.gt["foot_contacts"]
    assert (np.argmax(c, axis=1) == (np.arange(23) // 5) % 2).all()
    seen = seq.img_smpl.foot_contacts.numpy()
    assert (seen <= c).all() and seen.sum() == 4 * 1 + 0              # stances of 5 keep one frame, the last one of 3 none
    with pytest.raises(ValueError):
        make_sequence(tables, seed=1, num_frames=8, num_markers=8, planted_feet=True, stance_frames=0)


# ------------------------------------------------------------------------------------------------ 5. C entry point
def test_entry_point_is_declared_bound_and_typed_as_in_the_header(tmp_path):
    from uuo_mocap_amd import _lib

    assert "uuo_fit_set_foot_lock" in _lib.header_symbols()
    assert _lib._SIGNATURES["uuo_fit_set_foot_lock"] == (c_int, [c_void_p, c_float, c_void_p])
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+uuo_fit_set_foot_lock\s*\(\s*uuo_fit_t\s*\*\s*fit\s*,\s*float\s+w\s*,\s*const\s+float\s*\*\s*"
                     r"d_contacts\s*\)\s*;", text)
    src = tmp_path / "sig.c"
    src.write_text('#include "uuo_hip.h"\nint (*fp)(uuo_fit_t*, float, const float*) = uuo_fit_set_foot_lock;\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "sig.o")])
    assert _lib.ABI_VERSION == 3  # the problem structure and the ABI version did not change
    lib = _lib.load()             # (dlopen needs no GPU) bound with the declared types
    assert lib.uuo_fit_set_foot_lock.argtypes == [c_void_p, c_float, c_void_p] and lib.uuo_fit_set_foot_lock.restype == c_int


def test_units_note_in_the_header():
    from uuo_mocap_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    note = text[text.index("contact-gated foot-lock"):text.index("int uuo_fit_set_foot_lock")]
    assert "m^2 per frame^2" in note and "frame rate" in note and "d_contacts" in note
