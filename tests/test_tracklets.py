"""EXTENSION: tracklets of a capture whose marker columns change identity (uuo_mocap_amd/tracklets.py,
stages.compute_locations.tracklets) -- the segmentation rule on hand-written arrays and on the synthetic capture with identity
events, the generator's option, the config validation and every refusal that needs no device."""
import copy

import numpy as np
import pytest
import torch

from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.synthetic import make_sequence
from uuo_mocap_amd.tracklets import segment_tracklets, tracklets_config, tracklets_from_identity


def _column(xs):
    """[F, 1, 3] markers from a list of x coordinates (None = missing; y = 1 keeps a visible entry away from exact zeros)."""
    m = torch.zeros(len(xs), 1, 3)
    for f, x in enumerate(xs):
        if x is not None:
            m[f, 0] = torch.tensor([float(x), 1.0, 0.0])
    return m


def _seg(xs, max_gap=3, max_jump=0.25, min_length=1):
    return segment_tracklets(_column(xs), max_gap, max_jump, min_length)


# ------------------------------------------------------------------------------------------------ the rule, by hand
def test_gap_of_exactly_max_gap_joins_and_one_more_splits():
    t = _seg([0, 0, None, None, None, 0, 0], max_gap=3)
    assert t.seg[:, 0].tolist() == [0, 0, -1, -1, -1, 0, 0]
    assert (t.count, t.column.tolist(), t.start.tolist(), t.stop.tolist()) == (1, [0], [0], [7])
    t = _seg([0, 0, None, None, None, None, 0, 0], max_gap=3)
    assert t.seg[:, 0].tolist() == [0, 0, -1, -1, -1, -1, 1, 1]
    assert (t.start.tolist(), t.stop.tolist()) == ([0, 6], [2, 8])
    t = _seg([0, None, 0], max_gap=0)
    assert t.seg[:, 0].tolist() == [0, -1, 1]


def test_jump_scales_with_the_frames_since_the_previous_visible_entry():
    # max_jump 0.25 m per frame (exact in binary): across a gap of k = 2 missing frames the entry is 3 frames later
    for k in (0, 1, 2):
        at = 0.25 * (k + 1)
        xs = [0.0] + [None] * k
        assert _seg(xs + [at, at]).seg[:, 0].tolist() == [0] + [-1] * k + [0, 0], k          # exactly max_jump: same tracklet
        above = float(np.nextafter(np.float32(at), np.float32(10.0)))
        assert _seg(xs + [above, above]).seg[:, 0].tolist() == [0] + [-1] * k + [1, 1], k    # just above: a new one
    # the jump is the Euclidean norm of all three components
    m = _column([0, 0])
    m[1, 0] = torch.tensor([0.2, 1.2, 0.0])  # |(0.2, 0.2, 0)| = 0.283 > 0.25
    assert segment_tracklets(m, 3, 0.25, 1).seg[:, 0].tolist() == [0, 1]


def test_min_length_drops_a_tracklet_and_renumbers_the_rest():
    xs = [0, 0, 0, 5, 5, 9, 9, 9]
    t = _seg(xs, min_length=1)
    assert t.seg[:, 0].tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
    t = _seg(xs, min_length=3)
    assert t.seg[:, 0].tolist() == [0, 0, 0, -1, -1, 1, 1, 1]
    assert (t.count, t.start.tolist(), t.stop.tolist()) == (2, [0, 5], [3, 8])
    # the length counts visible entries, not the span
    t = _seg([0, None, 0, None, 0], min_length=3)
    assert t.seg[:, 0].tolist() == [0, -1, 0, -1, 0] and t.stop.tolist() == [5]
    assert _seg([0, None, 0, None, 0], min_length=4).count == 0


def test_ids_are_ordered_by_column_then_start_and_an_all_missing_column_has_none():
    m = torch.zeros(6, 3, 3)
    m[:, 0] = torch.tensor([0.0, 1.0, 0.0])
    m[3:, 0] = torch.tensor([5.0, 1.0, 0.0])          # column 0: two tracklets
    m[2:, 2] = torch.tensor([1.0, 1.0, 1.0])          # column 2: one, starting before column 0's second; column 1: nothing
    t = segment_tracklets(m, 3, 0.25, 1)
    assert t.seg.dtype == torch.int32
    assert t.seg.T.tolist() == [[0, 0, 0, 1, 1, 1], [-1] * 6, [-1, -1, 2, 2, 2, 2]]
    assert (t.column.tolist(), t.start.tolist(), t.stop.tolist()) == ([0, 0, 2], [0, 3, 2], [3, 6, 6])
    assert t.columns_with_events().tolist() == [True, False, False]
    empty = segment_tracklets(torch.zeros(4, 2, 3), 3, 0.25, 1)
    assert empty.count == 0 and bool((empty.seg == -1).all())


def test_single_frame():
    t = segment_tracklets(torch.tensor([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0]]]), 3, 0.1, 1)
    assert t.seg.tolist() == [[0, -1, 1]] and t.start.tolist() == [0, 0] and t.stop.tolist() == [1, 1]
    assert segment_tracklets(torch.ones(1, 2, 3), 3, 0.1, 2).count == 0


def test_parameters_are_checked():
    m = torch.ones(3, 1, 3)
    for bad in (dict(max_gap=-1), dict(max_gap=1.5), dict(min_length=0), dict(max_jump=0.0), dict(max_jump=float("inf")),
                dict(max_jump=float("nan")), dict(max_jump=-0.1)):
        kw = dict(max_gap=3, max_jump=0.1, min_length=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            segment_tracklets(m, **kw)
    with pytest.raises(ValueError):
        segment_tracklets(torch.ones(3, 3), 3, 0.1, 1)


# ------------------------------------------------------------------------------------------------ the generator
@pytest.fixture(scope="module")
def event_sequences(tables):
    return {seed: make_sequence(tables, seed=seed, num_frames=300, num_markers=50, identity_events=12, dropout=0.02)
            for seed in range(3)}


def test_zero_events_is_the_sequence_without_the_argument(tables):
    a = make_sequence(tables, seed=1, num_frames=40, num_markers=12)
    b = make_sequence(tables, seed=1, num_frames=40, num_markers=12, identity_events=0)
    assert np.array_equal(a.markers.get_points(), b.markers.get_points())
    for k in a.gt:
        assert np.array_equal(a.gt[k], b.gt[k]), k
    for k in ("trans", "root_orient", "pose_body", "betas", "foot_contacts", "img_mask"):
        assert torch.equal(getattr(a.img_smpl, k), getattr(b.img_smpl, k)), k
    # without events every visible entry shows the column's own vertex
    pts, vids = a.markers.get_points(), a.gt["marker_vids_fm"]
    vis = np.abs(pts).sum(-1) != 0
    assert np.array_equal(vids, np.where(vis, a.gt["marker_vids"][None, :], -1))
    assert np.array_equal(a.gt["tracklets_fm"] >= 0, vis)


def test_events_rotate_three_columns_and_leave_everything_else_alone(tables, event_sequences):
    seq = event_sequences[0]
    plain = make_sequence(tables, seed=0, num_frames=300, num_markers=50, dropout=0.02)
    pts, vids = seq.markers.get_points(), seq.gt["marker_vids_fm"]
    assert pts.shape == (300, 50, 3) and vids.shape == (300, 50) and seq.gt["tracklets_fm"].shape == (300, 50)
    for k in ("verts", "joints", "rot", "betas", "trans", "marker_vids", "marker_offsets"):
        assert np.array_equal(seq.gt[k], plain.gt[k]), k
    assert np.array_equal(pts[:25], plain.markers.get_points()[:25])        # no event before F / 10, no blank 5 frames before that
    vis = np.abs(pts).sum(-1) != 0
    assert np.array_equal(vids >= 0, vis)
    # every visible entry sits 9.5 mm (+ 1 mm noise) off the vertex that gt names
    d = np.linalg.norm(pts - np.take_along_axis(seq.gt["verts"], np.maximum(vids, 0)[..., None], axis=1), axis=-1)
    assert float(d[vis].max()) < 0.02
    # ... and some columns do change identity, in a way the per-column table does not know
    changed = (vids != seq.gt["marker_vids"][None, :]) & vis
    assert changed.any(axis=0).sum() >= 3
    # in a frame without blanks the columns are a permutation of the plain capture's
    f = 299
    assert sorted(vids[f][vis[f]].tolist()) == sorted(plain.gt["marker_vids_fm"][f][plain.gt["marker_vids_fm"][f] >= 0].tolist())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_segmentation_recovers_the_true_tracklets(event_sequences, seed):
    """The shipped parameters on the 300 x 50 capture with 12 identity events and block dropout: `seg` equals the generator's
    tracklets, after the same min_length on both.  (The generator's own motion stays below 0.078 m per frame on these seeds,
    under max_jump = 0.1.)"""
    p = tracklets_config(packaged_config("video_mocap_tracklets"))
    assert p == {"max_gap": 3, "max_jump": 0.1, "min_length": 10}
    seq = event_sequences[seed]
    got = segment_tracklets(torch.from_numpy(seq.markers.get_points()), **p)
    want = tracklets_from_identity(torch.from_numpy(seq.gt["tracklets_fm"]), p["min_length"])
    assert got.count == want.count and got.count > 50
    assert torch.equal(got.seg, want.seg)
    assert torch.equal(got.column, want.column) and torch.equal(got.start, want.start) and torch.equal(got.stop, want.stop)
    assert int(got.columns_with_events().sum()) >= 3


# ------------------------------------------------------------------------------------------------ config
def test_config_key_is_off_when_absent_and_validated_with_its_path():
    assert tracklets_config(packaged_config("video_mocap")) is None
    cfg = packaged_config("video_mocap_tracklets")
    base = packaged_config("video_mocap")
    rest = copy.deepcopy(cfg)
    del rest["stages"]["compute_locations"]["tracklets"]
    rest["name"], rest["parent"] = base["name"], base["parent"]
    assert rest == base                                                      # video_mocap.yaml plus the key, nothing else
    for bad in ({"max_gap": -1}, {"max_gap": 2.5}, {"max_gap": True}, {"min_length": 0}, {"min_length": 1.5}, {"max_jump": 0},
                {"max_jump": float("inf")}, {"max_jump": float("nan")}, {"max_jump": "fast"}):
        c = copy.deepcopy(cfg)
        c["stages"]["compute_locations"]["tracklets"].update(bad)
        with pytest.raises(ValueError, match=r"stages\.compute_locations\.tracklets"):
            tracklets_config(c)
    for bad in ({"max_gap": 3, "max_jump": 0.1}, {"max_gap": 3, "max_jump": 0.1, "min_length": 10, "extra": 1}, [3, 0.1, 10], 5):
        c = copy.deepcopy(cfg)
        c["stages"]["compute_locations"]["tracklets"] = bad
        with pytest.raises(ValueError, match=r"stages\.compute_locations\.tracklets"):
            tracklets_config(c)
    c = copy.deepcopy(cfg)
    c["stages"]["compute_locations"]["tracklets"] = None
    assert tracklets_config(c) is None


def test_lockstep_batches_are_not_offered_with_the_key():
    from uuo_mocap_amd import optimization

    assert optimization.lockstep_supported(packaged_config("video_mocap"), "marker")
    assert not optimization.lockstep_supported(packaged_config("video_mocap_tracklets"), "marker")
    assert optimization.lockstep_supported(packaged_config("video_mocap_tracklets"), "chamfer")


# ------------------------------------------------------------------------------------------------ refusals without a device
class _NoDeviceSmpl:
    """Stands where a SmplInference goes in calls that must refuse before anything reaches the device."""

    class device_model:
        V = 6890


def _call_optim_markers(cfg, frame_assign, **patches):
    from uuo_mocap_amd import optimization, parallel

    F, M = 4, 3
    z = torch.zeros
    old = {k: getattr(parallel, k) for k in patches}
    try:
        for k, v in patches.items():
            setattr(parallel, k, v)
        optimization.optim_markers(markers=z(F, M, 3), pose_body=z(F, 23, 3, 3), o_pose_body=z(F, 23, 3, 3), betas=z(1, 10),
                                   o_betas=z(1, 10), root_orient=z(F, 1, 3, 3), trans=z(F, 3), barycentric_coords_one_hot=None,
                                   img_mask=torch.ones(F), smpl_inference=_NoDeviceSmpl(), config=cfg, frame_assign=frame_assign)
    finally:
        for k, v in old.items():
            setattr(parallel, k, v)


def test_routes_that_cannot_carry_the_table_refuse_it_up_front():
    table = torch.zeros(4, 3, dtype=torch.int32)
    cfg = packaged_config("video_mocap_tracklets")
    c = copy.deepcopy(cfg)
    c["stages"]["marker"]["losses"]["latent_offsets"] = 1.0
    with pytest.raises(NotImplementedError, match="latent"):
        _call_optim_markers(c, table)
    c = copy.deepcopy(cfg)
    c["stages"]["marker"]["robust_sigma"] = 0.05
    c["execution"] = {"robust_fused": False}
    with pytest.raises(NotImplementedError, match="composed from the operators"):
        _call_optim_markers(c, table)
    c = copy.deepcopy(cfg)
    c["stages"]["marker"]["losses"]["joint_accel"] = 1.0
    c["execution"] = {"temporal_fused": False}
    with pytest.raises(NotImplementedError, match="composed from the operators"):
        _call_optim_markers(c, table)

    class _Shard:
        active = True

    with pytest.raises(NotImplementedError, match="frame-block sharding"):
        _call_optim_markers(cfg, table, frame_shard=lambda: _Shard())
    with pytest.raises(NotImplementedError, match="shared betas"):
        _call_optim_markers(cfg, table, shared_betas_reducer=lambda: object())


def test_solve_batch_refuses_problems_with_a_table():
    from uuo_mocap_amd import engine

    class _P:
        joint_accel = 0.0
        foot_lock = 0.0
        surface = False
        frame_assign = torch.zeros(2, 2, dtype=torch.int32)
        model = None

        class problem:
            w_offsets = 0.0

    with pytest.raises(NotImplementedError, match="per-frame vertex table"):
        engine.solve_batch([_P()], [torch.zeros(1)], max_iter=1)
