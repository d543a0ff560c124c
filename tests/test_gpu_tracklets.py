"""EXTENSION: per-tracklet marker placement for captures whose columns change identity, on the MI355X -- the segmented placement
kernel (uuo_assign_segments_argmin) against a numpy fp32 restatement of its rule, the marker closure on a per-frame vertex table
(uuo_fit_set_frame_assign) against float64 autograd, the table switched off, the placement on the true body and the fit of
video_mocap_tracklets.yaml on a capture with identity events."""
import copy
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from oracle import stages_ref  # noqa: E402
from foot_lock_ref64 import _contacts  # noqa: E402
from gpu_support import (W_ACCEL_M as W_ACCEL, W_LOCK_M as W_LOCK, _fit, _inputs, _rel_err, _vertex_error, dev,  # noqa: E402,F401
                         smpl, smpl64)
from stage_ref64 import _accel64, _d64, _float64, _lock64, _rho  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402
from uuo_mocap_amd.tracklets import Tracklets, segment_tracklets, tracklets_config  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. the placement kernel
def _segments_ref(verts, markers, seg, valid, S):
    """The rule, restated: an elementwise float32 loop over the frames.  norm = sqrt((dx dx + dy dy) + dz dz), the sum
    sequential in f, one divide by the count of the frames summed, lowest vertex id on ties, -1 without a summed frame."""
    F, V, _ = verts.shape
    acc = np.zeros((S, V), np.float32)
    n = np.zeros(S, np.int64)
    for f in range(F):
        if not valid[f]:
            continue
        for m in range(markers.shape[1]):
            s = int(seg[f, m])
            if s < 0:
                continue
            dx, dy, dz = (verts[f, :, c] - markers[f, m, c] for c in range(3))
            acc[s] = acc[s] + np.sqrt((dx * dx + dy * dy) + dz * dz)
            n[s] += 1
    assert acc.dtype == np.float32
    return np.array([int(np.argmin(acc[s] / np.float32(n[s]))) if n[s] else -1 for s in range(S)], np.int32)


def _kernel_case(F, M, V, seed):
    """verts, markers, seg, valid with: tracklet boundaries at frames 31 | 32 | 33 (column 0: a tracklet of length 1 at 31 and one
    at 32), a boundary inside a group of four frames and -1 entries inside a run (column 1), a column with no tracklet (2), a
    tracklet whose frames are all invalid (column 3), a whole column on a duplicated vertex (4), random cuts (5 and up)."""
    rng = np.random.default_rng(seed)
    verts = rng.normal(size=(F, V, 3)).astype(np.float32)
    verts[:, 5] = verts[:, 200]          # duplicated vertices: exact ties
    verts[:, 0] = verts[:, V - 1]
    markers = rng.normal(size=(F, M, 3)).astype(np.float32)
    runs = {m: [] for m in range(M)}     # column -> list of (first frame, one past the last)
    runs[0] = [(0, 31), (31, 32), (32, 33), (33, F)]
    if M > 1:
        runs[1] = [(0, 6), (6, F)]
    if M > 3:
        runs[3] = [(10, 14), (20, F)]
    if M > 4:
        runs[4] = [(0, F)]
        markers[:, 4] = verts[:, 200] + 1e-3 * rng.normal(size=(F, 3)).astype(np.float32)   # the winner is the duplicated pair
    for m in range(5, M):
        cuts = sorted(set(rng.integers(1, max(F, 2), size=3).tolist()))
        runs[m] = list(zip([0] + cuts, cuts + [F]))
    seg = np.full((F, M), -1, np.int32)
    S = 0
    for m in range(M):
        for a, b in runs[m]:
            a, b = min(a, F), min(b, F)
            if b > a:
                seg[a:b, m] = S
                S += 1
    if M > 1 and F > 4:
        seg[2:4, 1] = -1                 # missing entries inside a run
        markers[2:4, 1] = 0.0
    valid = np.ones(F, np.uint8)
    valid[10:14] = 0                     # column 3's first tracklet has no valid frame; others lose four frames
    if F > 40:
        valid[40] = 0
    return verts, markers, seg, valid, S


@pytest.mark.parametrize("V", [257, 6890])
@pytest.mark.parametrize("M", [1, 5, 9])
@pytest.mark.parametrize("F", [1, 33, 70])
def test_segment_kernel_matches_the_fp32_restatement(smpl, dev, F, M, V):
    verts, markers, seg, valid, S = _kernel_case(F, M, V, 1000 * F + 10 * M + (V == 257))
    want = _segments_ref(verts, markers, seg, valid, S)
    got = smpl.device_model.assign_segments_argmin(torch.from_numpy(verts).to(dev), torch.from_numpy(markers).to(dev),
                                                   torch.from_numpy(seg).to(dev), torch.from_numpy(valid).to(dev), S)
    assert got.dtype == torch.int32 and tuple(got.shape) == (S,)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    if F >= 33:
        assert S >= 3 and (seg[31, 0], seg[32, 0]) == (1, 2)
    if F == 70 and M >= 5:
        s3 = int(seg[10, 3])
        assert want[s3] == -1                                # every frame of this tracklet is invalid
        assert want[int(seg[0, 4])] == 5                     # vertices 5 and 200 tie: the lower id


@pytest.mark.parametrize("F,M,V", [(70, 9, 257), (33, 50, 6890)])
def test_one_tracklet_per_column_is_the_column_placement(smpl, dev, F, M, V):
    rng = np.random.default_rng(F + M)
    verts = torch.from_numpy(rng.normal(size=(F, V, 3)).astype(np.float32)).to(dev)
    verts[:, 7] = verts[:, 100]
    markers = torch.from_numpy(rng.normal(size=(F, M, 3)).astype(np.float32)).to(dev)
    markers[:, 0] = verts[:, 100]
    valid = torch.ones(F, dtype=torch.bool, device=dev)
    seg = torch.arange(M, dtype=torch.int32, device=dev)[None, :].expand(F, M).contiguous()
    dm = smpl.device_model
    a = dm.assign_segments_argmin(verts, markers, seg, valid, M)
    b = dm.assign_mean_argmin(verts, markers, valid)
    assert torch.equal(a, b) and int(a[0]) == 7


# ------------------------------------------------------------------------------------------------ 2. the closure
def _cfg(sigma=0.0, temporal=False):
    cfg = packaged_config("video_mocap")
    st = cfg["stages"]["marker"]
    st["robust_sigma"] = sigma
    if temporal:
        st["losses"]["joint_accel"] = W_ACCEL
        st["losses"]["foot_lock"] = W_LOCK
    return cfg


VARIANTS = {"plain": dict(), "robust": dict(sigma=0.05), "accel+lock": dict(temporal=True)}


def _table(seq, F, M, seed):
    """[F, M] int32: the true vertices, with vertex changes inside the frames one block walks (every column changes at least
    once when F > 1) and -1 entries."""
    gen = torch.Generator().manual_seed(seed)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    table = vids[None, :].repeat(F, 1)
    other = torch.randint(0, 6890, (F, M), generator=gen)
    cut = torch.randint(1, max(F, 2), (M,), generator=gen)
    frame = torch.arange(F)[:, None]
    table = torch.where(frame >= cut[None, :], other[0][None, :].expand(F, M), table)
    table = torch.where(torch.rand(F, M, generator=gen) < 0.1, other, table)          # single-frame changes
    table = torch.where(torch.rand(F, M, generator=gen) < 0.15, torch.full_like(table, -1), table)
    table[F - 1, 0] = -1
    return table.to(torch.int32)


def _ref_marker_table(smpl64, cfg, markers, o_pose, o_betas, x, table, contacts):
    """The marker stage on a per-frame vertex table in float64 autograd: item (f, m) is vertex table[f, m], an entry < 0 has
    weight 0; everything else is the per-column closure."""
    from uuo_mocap_amd.engine import MARKER_DISTANCE

    F = markers.shape[0]
    st = cfg["stages"]["marker"]
    w, sigma = st["losses"], float(st.get("robust_sigma", 0.0))
    with _float64():
        x = x.detach().cpu().double()
        markers, o_pose, o_betas = _d64(markers, o_pose, o_betas)
        leaves = [t.clone().requires_grad_(True) for t in (x[:207 * F].reshape(F, 23, 3, 3), x[207 * F:207 * F + 10].reshape(1, 10),
                                                          x[207 * F + 10:216 * F + 10].reshape(F, 1, 3, 3),
                                                          x[216 * F + 10:].reshape(F, 3))]
        pose, betas, root, trans = leaves
        out = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(pose), betas, stages_ref.normalize_rot(root), trans)
        t = table.cpu().long()
        vm = torch.gather(out["vertices"], 1, t.clamp(min=0)[..., None].expand(-1, -1, 3))
        weight = stages_ref.get_marker_mask(markers).double() * (t >= 0).double()
        e = torch.norm(markers - vm, dim=-1) - MARKER_DISTANCE
        loss = torch.mean(_rho(e ** 2, sigma) * weight) * w["marker"] + Fn.mse_loss(pose, o_pose) * w["reg_pose_body"] + \
            Fn.mse_loss(betas, o_betas) * w["reg_betas"]
        if "joint_accel" in w:
            loss = loss + _accel64(out["joints"]) * w["joint_accel"] + _lock64(out["joints"][:, :24], contacts) * w["foot_lock"]
        loss.backward()
    return float(loss.detach()), torch.cat([g.grad.reshape(-1) for g in leaves]).numpy()


def _problem(smpl, dev, cfg, markers, o_pose, o_betas, contacts, assign=None, table=None):
    from uuo_mocap_amd.engine import MarkerProblem

    return MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), None if assign is None else assign.to(dev), cfg,
                         foot_contacts=contacts, frame_assign=None if table is None else table.to(dev))


@pytest.mark.parametrize("M", [1, 7, 50])
@pytest.mark.parametrize("F", [3, 17])
def test_table_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, M):
    """Tolerances: those of the float64 checks of the per-column marker closure (test_gpu_temporal, test_gpu_foot_lock)."""
    seq, markers, o_pose, o_betas, root, trans, (tp, _, bp, pp, rp) = _inputs(tables, F, 300 + 10 * F + M, num_markers=M)
    table = _table(seq, F, M, F * M)
    assert bool((table < 0).any()) and bool((table[1:] != table[:-1]).any())
    contacts = _contacts(F, F)
    for name, kw in VARIANTS.items():
        cfg = _cfg(**kw)
        prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, contacts, table=table)
        assert prob.n == 219 * F + 10
        x = prob.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        loss, grad, _ = prob.evaluate(x, want_nn=False)
        lo, g_ref = _ref_marker_table(smpl64, cfg, markers, o_pose, o_betas, x, table, contacts)
        err = _rel_err(grad.cpu().numpy(), g_ref)
        print("OBS table closure parity (%s, F %d, M %d): loss rel %.2e, gradient rel %.2e" % (name, F, M, abs(loss - lo) / abs(lo), err))
        np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=name)
        assert err < 2e-4, name


def _eval_and_solve(prob, x0, iters=5):
    loss, grad, _ = prob.evaluate(x0, want_nn=False)
    x = x0.clone()
    stats = prob.solve(x, max_iter=iters)
    torch.cuda.synchronize()
    return loss, grad.clone(), x, stats["final_loss"], stats["n_eval"]


def _same(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3:] == b[3:]


def test_constant_table_is_the_column_path_bit_for_bit(smpl, tables, dev):
    F, M = 17, 50
    seq, markers, o_pose, o_betas, root, trans, (tp, _, bp, pp, rp) = _inputs(tables, F, 41)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    contacts = _contacts(F, 3)
    for name, kw in VARIANTS.items():
        cfg = _cfg(**kw)
        col = _problem(smpl, dev, cfg, markers, o_pose, o_betas, contacts, assign=vids)
        tab = _problem(smpl, dev, cfg, markers, o_pose, o_betas, contacts, table=vids[None, :].repeat(F, 1))
        x0 = col.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        assert _same(_eval_and_solve(tab, x0), _eval_and_solve(col, x0)), name


def test_negative_entries_are_zeroed_markers(smpl, tables, dev):
    F, M = 17, 50
    seq, markers, o_pose, o_betas, root, trans, (tp, _, bp, pp, rp) = _inputs(tables, F, 43)
    table = _table(seq, F, M, 7)
    off = table < 0
    assert int(off.sum()) > 20
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    filled = torch.where(off, vids[None, :].expand(F, M), table)
    zeroed = markers.clone()
    zeroed[off] = 0.0
    contacts = _contacts(F, 5)
    for name, kw in VARIANTS.items():
        cfg = _cfg(**kw)
        a = _problem(smpl, dev, cfg, markers, o_pose, o_betas, contacts, table=table)
        b = _problem(smpl, dev, cfg, zeroed, o_pose, o_betas, contacts, table=filled)
        x0 = a.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        assert _same(_eval_and_solve(a, x0), _eval_and_solve(b, x0)), name


def test_plain_problems_on_the_shared_workspace_are_untouched_and_runs_repeat(smpl, tables, dev):
    F, M = 17, 50
    seq, markers, o_pose, o_betas, root, trans, (tp, _, bp, pp, rp) = _inputs(tables, F, 47)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    table = _table(seq, F, M, 11)
    cfg = _cfg()
    fresh = {}

    def on_fresh_thread():   # a workspace of its own (workspaces are per thread) that never saw a table
        p = _problem(smpl, dev, cfg, markers, o_pose, o_betas, None, assign=vids)
        fresh["plain"] = _eval_and_solve(p, p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev)))

    t = threading.Thread(target=on_fresh_thread)
    t.start()
    t.join()
    tab = _problem(smpl, dev, cfg, markers, o_pose, o_betas, None, table=table)
    col = _problem(smpl, dev, cfg, markers, o_pose, o_betas, None, assign=vids)
    assert tab.fit.value == col.fit.value                     # one (F, M) workspace for both
    x0 = col.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    first = _eval_and_solve(tab, x0)
    plain = _eval_and_solve(col, x0)
    again = _eval_and_solve(tab, x0)
    assert _same(plain, fresh["plain"])
    assert _same(first, again)
    assert not _same(first, plain)


def test_library_refuses_the_table_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F, M = 5, 7
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 3, num_markers=M)
    table = _table(seq, F, M, 1).to(dev)
    cfg = packaged_config("video_mocap")
    ch = ChamferProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    ch.frame_assign = table            # (no public route sets it on a chamfer problem: the library's own refusal)
    with pytest.raises(RuntimeError, match="marker stage only"):
        ch.evaluate(ch.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev)))
    ch.frame_assign = None
    ch.evaluate(ch.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev)))
    offs = copy.deepcopy(cfg)
    offs["stages"]["marker"]["losses"]["latent_offsets"] = 1.0
    with pytest.raises(NotImplementedError, match="latent marker offsets"):
        MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), None, offs, frame_assign=table)
    with pytest.raises(NotImplementedError, match="three-corner"):
        MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), torch.zeros(M, 3, dtype=torch.int32), cfg,
                      bary=torch.full((M, 3), 1.0 / 3.0), frame_assign=table)
    with pytest.raises(ValueError, match="frame_assign"):
        MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), None, cfg, frame_assign=table[:, :3])
    po = MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), torch.zeros(M, dtype=torch.int32), offs)
    po.frame_assign = table
    with pytest.raises(RuntimeError, match="latent marker offsets"):
        po.evaluate(po.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev)), want_nn=False)


# ------------------------------------------------------------------------------------------------ 3. placement and fit
@pytest.fixture(scope="module")
def capture(tables):
    return make_sequence(tables, seed=0, num_frames=300, num_markers=50, identity_events=12, dropout=0.02)


def _rest_distance(tables, a, b):
    vt = torch.from_numpy(np.asarray(tables.v_template)).float()
    return (vt[a.long().clamp(min=0)] - vt[b.long().clamp(min=0)]).norm(dim=-1)


def test_placement_on_the_true_body(smpl, tables, dev, capture, record_property):
    """On the ground-truth body every tracklet of >= 10 frames of the 12-event capture lands within 2.5 cm (rest pose) of its
    true vertex.  The whole-column placement (compute_nearest_points) is recorded beside it for the columns with events."""
    from uuo_mocap_amd.optimization import compute_nearest_points, compute_tracklet_placement

    seq = capture
    cfg = packaged_config("video_mocap_tracklets")
    markers = torch.from_numpy(seq.markers.get_points()).float().to(dev)
    trk = segment_tracklets(markers, **tracklets_config(cfg))
    rot = torch.from_numpy(seq.gt["rot"]).float().to(dev)
    betas = torch.from_numpy(seq.gt["betas"]).float().to(dev)
    trans = torch.from_numpy(seq.gt["trans"]).float().to(dev)
    mask = seq.img_smpl.img_mask.to(dev)
    table = compute_tracklet_placement(markers, rot[:, 1:], betas, rot[:, :1], trans, smpl, mask, trk).cpu()
    assert table.dtype == torch.int32 and tuple(table.shape) == (300, 50)
    seg = trk.seg.cpu()
    assert torch.equal(table >= 0, seg >= 0)
    true = torch.from_numpy(seq.gt["marker_vids_fm"])
    d = _rest_distance(tables, table, true)
    worst = float(d[seg >= 0].max())
    for s in range(trk.count):                                # one vertex per tracklet
        assert int(table[seg == s].unique().numel()) == 1
    one_hot = compute_nearest_points(markers=markers, pose_body=rot[:, 1:], betas=betas, root_orient=rot[:, :1], trans=trans,
                                     smpl_inference=smpl, marker_labels=None, granularity="full", img_mask=mask, device=dev,
                                     config=cfg)
    col = torch.argmax(one_hot, dim=-1).cpu()
    events = trk.columns_with_events().cpu()
    vis = true >= 0
    dc = _rest_distance(tables, col[None, :].expand(300, 50), true)
    col_events = dc[:, events][vis[:, events]]
    print("OBS placement on the true body: %d tracklets, worst %.2f mm; whole-column placement on the %d columns with more than "
          "one tracklet: mean %.1f mm, worst %.1f mm over their visible entries"
          % (trk.count, 1e3 * worst, int(events.sum()), 1e3 * float(col_events.mean()), 1e3 * float(col_events.max())))
    record_property("tracklet_worst_m", worst)
    record_property("column_mean_m", float(col_events.mean()))
    assert worst <= 0.025


def test_fit_of_a_capture_with_identity_events(smpl, oracle_smpl, tables, dev, capture, record_property):
    """300 x 50, seed 0, mean vertex error against gt["verts"]: (a) the clean capture under video_mocap.yaml, (b) the 12-event
    capture under video_mocap.yaml, (c) the 12-event capture under video_mocap_tracklets.yaml.  Required: c <= a + 0.5 mm and
    c < b."""
    clean = make_sequence(tables, seed=0, num_frames=300, num_markers=50, dropout=0.02)
    out_a = _fit(clean, "video_mocap", smpl, dev)
    out_b = _fit(capture, "video_mocap", smpl, dev)
    out_c = _fit(capture, "video_mocap_tracklets", smpl, dev)
    a, b, c = (_vertex_error(o, s, oracle_smpl) for o, s in ((out_a, clean), (out_b, capture), (out_c, capture)))
    assert "marker_vertices" not in out_a and "marker_tracklets" not in out_b
    mv, mt = out_c["marker_vertices"], out_c["marker_tracklets"]
    assert mv.dtype == torch.int32 and mt.dtype == torch.int32 and tuple(mv.shape) == tuple(mt.shape) == (300, 50)
    assert torch.equal(mv >= 0, mt >= 0)
    true = torch.from_numpy(capture.gt["marker_vids_fm"])
    placed = mt >= 0
    share = float((_rest_distance(tables, mv, true)[placed] <= 0.025).float().mean())
    labels = np.asarray(out_c["markers_labels"])
    assert labels.shape == (300, 50)
    print("OBS identity events 300 x 50: vertex error clean/plain %.2f mm, events/plain %.2f mm, events/tracklets %.2f mm; %.1f %% of "
          "the placed entries within 2.5 cm (rest pose) of their true vertex; %.1f %% of the visible entries placed"
          % (1e3 * a, 1e3 * b, 1e3 * c, 100.0 * share, 100.0 * float(placed.sum()) / float((true >= 0).sum())))
    for k, v in (("a_m", a), ("b_m", b), ("c_m", c), ("share_within_25mm", share)):
        record_property(k, v)
    assert c < b, (a, b, c)
    assert c <= a + 5e-4, (a, b, c)
