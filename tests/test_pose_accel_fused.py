"""EXTENSION: the pose-acceleration term on the fused chamfer and marker closures (execution.pose_accel_fused, opt-in;
k_pose_accel, uuo_fit_set_pose_accel) -- what needs no device: the switch and its default, the route decision with it on and
off, the refusals that stay (frame-block sharding, lock-step batches, the soft-assignment closure), the shipped config against
its parent, and the new symbol in the header, the export map and the ctypes table.  tests/test_gpu_pose_accel_fused.py holds the
kernel's checks."""
import fnmatch
import os
import re

import pytest

from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.terms import POSE_ACCEL, TERMS, StageTerms, lockstep_supported, stage_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "pose_accel_fused"


def _cfg(name="video_mocap", switch=None, **stages):
    """packaged config; `switch` (None = absent) goes to execution.pose_accel_fused, per stage a dict of losses"""
    cfg = packaged_config(name)
    if switch is not None:
        cfg["execution"] = dict(cfg.get("execution") or {}, **{SWITCH: switch})
    for stage, kv in stages.items():
        cfg["stages"][stage]["losses"].update(kv)
    return cfg


def test_the_switch_parses_and_is_off_when_absent():
    from uuo_mocap_amd.markers_utils import EXECUTION_DEFAULTS, merge_execution

    assert POSE_ACCEL.switch == SWITCH and POSE_ACCEL.opt_in and TERMS[-1] is POSE_ACCEL
    assert [t.label for t in TERMS if t.opt_in] == ["pose_accel"]          # the one switch whose default is off
    assert EXECUTION_DEFAULTS[SWITCH] is False
    assert merge_execution({"execution": {SWITCH: True}})[SWITCH] is True   # a known option of the runners
    for stage in ("chamfer", "marker"):
        on = {stage: {"pose_accel": 3.0}}
        assert not StageTerms(_cfg(**on), stage).fused(POSE_ACCEL)
        assert not StageTerms(_cfg(switch=False, **on), stage).fused(POSE_ACCEL)
        assert StageTerms(_cfg(switch=True, **on), stage).fused(POSE_ACCEL)
        assert StageTerms(_cfg(), stage).fused(POSE_ACCEL)                 # nothing to compose without the term
        assert StageTerms(_cfg(switch=False, **{stage: {"pose_accel": 0.0}}), stage).fused(POSE_ACCEL)


@pytest.mark.parametrize("on_device", [True, False])
def test_stage_route_answers_fused_with_the_switch_on(on_device):
    """both stages, markers / placement on the host and on the device; the marker stage's one-hot, three-corner and per-frame
    table placements.  (A three-corner placement has its fused closure on the device only: on the host it stays composed, with
    or without the term.)"""
    for cfg in (_cfg("video_mocap_rotsmooth_fused"), _cfg("video_mocap_rotsmooth", switch=True),
                _cfg(switch=True, chamfer={"pose_accel": 2.0}, marker={"pose_accel": 2.0})):
        assert stage_route(StageTerms(cfg, "chamfer"), on_device=on_device, sharded=False) == "fused"
        for placement in ("one_hot", "three", "frame_table"):
            want = "fused" if on_device or placement != "three" else "composed"
            assert stage_route(StageTerms(cfg, "marker"), on_device=on_device, sharded=False, placement=placement) == want
    for cfg in (_cfg("video_mocap_rotsmooth"), _cfg("video_mocap_rotsmooth", switch=False)):
        assert stage_route(StageTerms(cfg, "chamfer"), on_device=on_device, sharded=False) == "composed"
        for placement in ("one_hot", "three"):
            assert stage_route(StageTerms(cfg, "marker"), on_device=on_device, sharded=False, placement=placement) == "composed"
        with pytest.raises(NotImplementedError, match="per-frame vertex table"):
            stage_route(StageTerms(cfg, "marker"), on_device=on_device, sharded=False, placement="frame_table")


def test_the_stage_problems_take_the_term_only_with_the_switch():
    """without the switch the constructors refuse as they always have; with it they get past the terms' checks (and fail on the
    missing markers here: no device is touched)"""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    for stage, make in (("chamfer", lambda c: ChamferProblem(None, None, None, None, None, c)),
                        ("marker", lambda c: MarkerProblem(None, None, None, None, None, c))):
        on = {stage: {"pose_accel": 1.0}}
        for sw in (None, False):
            with pytest.raises(NotImplementedError, match="pose_accel.*no fused closure"):
                make(_cfg(switch=sw, **on))
        with pytest.raises(AttributeError):   # past the refusals: the first use of the (absent) body model or markers
            make(_cfg(switch=True, **on))
    with pytest.raises(NotImplementedError, match="pose_accel.*soft-assignment closure"):
        ChamferProblem(None, None, None, None, None, _cfg(switch=True, chamfer={"pose_accel": 1.0, "soft_chamfer": 10.0}))
    # beside soft_chamfer the call goes to the composed closure, switch or not
    for sw in (None, True):
        soft = _cfg(switch=sw, chamfer={"pose_accel": 1.0, "soft_chamfer": 10.0})
        assert stage_route(StageTerms(soft, "chamfer"), on_device=True, sharded=False) == "composed"


def test_sharding_and_lockstep_still_refuse():
    for sw in (None, True):
        cfg = _cfg("video_mocap_rotsmooth", switch=sw)
        with pytest.raises(NotImplementedError, match="pose_accel.*frame-block sharding"):
            stage_route(StageTerms(cfg, "chamfer"), on_device=True, sharded=True)
        for placement in ("one_hot", "three"):
            with pytest.raises(NotImplementedError, match="pose_accel.*frame-block sharding"):
                stage_route(StageTerms(cfg, "marker"), on_device=True, sharded=True, placement=placement)
        for stage in ("chamfer", "marker"):
            assert not lockstep_supported(cfg, stage)
    assert not lockstep_supported(_cfg("video_mocap_rotsmooth_fused"), "chamfer")
    assert lockstep_supported(_cfg(switch=True), "chamfer") and lockstep_supported(_cfg(switch=True), "marker")   # the switch alone
    # a problem that carries the term is refused by solve_batch before anything else is looked at
    from uuo_mocap_amd.engine import solve_batch

    class _Carries:
        model = None
        pacc_w = 2.0
        pose_accel_on = True

    with pytest.raises(NotImplementedError, match="lock-step batches do not carry the pose-acceleration term"):
        solve_batch([_Carries()], [None], max_iter=1)


def test_the_shipped_config_differs_from_its_parent_only_by_the_switch():
    parent, fused = packaged_config("video_mocap_rotsmooth"), packaged_config("video_mocap_rotsmooth_fused")
    assert fused["execution"][SWITCH] is True
    assert {k: v for k, v in fused["execution"].items() if k != SWITCH} == (parent.get("execution") or {})
    strip = lambda c: {k: v for k, v in c.items() if k not in ("execution", "name", "parent")}
    assert strip(fused) == strip(parent)


def test_the_symbol_is_in_the_header_the_export_map_and_the_ctypes_table():
    from uuo_mocap_amd import _lib

    name = "uuo_fit_set_pose_accel"
    header = open(os.path.join(ROOT, "include", "uuo_hip.h")).read()
    assert re.search(r"\bint %s\(uuo_fit_t\* fit, float w, const float\* h_joint_weights\);" % name, header)
    assert name in _lib.header_symbols() and name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES[name][1]) == 3
    exports = open(os.path.join(ROOT, "uuo_mocap_amd", "csrc", "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:(.*?);", exports, re.S).group(1).split(",")]
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert POSE_ACCEL.setter == name
