"""Deterministic synthetic mocap sequences (SURVEY.md 8d recipe) and the two input duck-types the
orchestrator consumes (reference img_smpl/img_smpl.py:26-31,100-132 ``ImgSmpl`` fields and
markers/markers.py:35-54 ``Markers`` accessors).

Data tooling, not the fitted path: ground-truth vertices come from a float64 numpy evaluation of the
SMPL equations so the generated inputs do not depend on either the HIP kernels or the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .body_model import NUM_JOINTS, SmplTables, hash_normal, hash_uniform


def _rodrigues(aa: np.ndarray) -> np.ndarray:
    """axis-angle [...,3] -> rotation matrices [...,3,3] (float64)."""
    theta = np.linalg.norm(aa, axis=-1, keepdims=True)
    k = aa / np.maximum(theta, 1e-12)
    kx, ky, kz = k[..., 0], k[..., 1], k[..., 2]
    zero = np.zeros_like(kx)
    K = np.stack([zero, -kz, ky, kz, zero, -kx, -ky, kx, zero], axis=-1).reshape(aa.shape[:-1] + (3, 3))
    s = np.sin(theta)[..., None]
    c = np.cos(theta)[..., None]
    eye = np.broadcast_to(np.eye(3), K.shape)
    return eye + s * K + (1.0 - c) * (K @ K)


def lbs_f64(tables: SmplTables, rot: np.ndarray, betas: np.ndarray, trans: np.ndarray):
    """SMPL forward in float64 numpy. rot [F,24,3,3], betas [F,10] or [1,10], trans [F,3].
    Returns verts [F,V,3], joints [F,24,3], per-vertex blended rotations [F,V,3,3]."""
    F = rot.shape[0]
    vt = tables.v_template.astype(np.float64)
    S = tables.shapedirs.astype(np.float64)
    P = tables.posedirs.astype(np.float64)
    Jr = tables.J_regressor.astype(np.float64)
    W = tables.lbs_weights.astype(np.float64)
    parents = tables.parents
    betas = np.broadcast_to(betas.astype(np.float64), (F, 10))
    v_shaped = vt[None] + np.einsum("bl,mkl->bmk", betas, S)
    J = np.einsum("bik,ji->bjk", v_shaped, Jr)
    pf = (rot[:, 1:] - np.eye(3)).reshape(F, -1)
    v_posed = v_shaped + (pf @ P).reshape(F, -1, 3)
    G_R = np.zeros((F, NUM_JOINTS, 3, 3))
    G_t = np.zeros((F, NUM_JOINTS, 3))
    G_R[:, 0] = rot[:, 0]
    G_t[:, 0] = J[:, 0]
    for j in range(1, NUM_JOINTS):
        p = parents[j]
        G_R[:, j] = G_R[:, p] @ rot[:, j]
        G_t[:, j] = np.einsum("fab,fb->fa", G_R[:, p], J[:, j] - J[:, p]) + G_t[:, p]
    A_t = G_t - np.einsum("fjab,fjb->fja", G_R, J)
    T_R = np.einsum("vj,fjab->fvab", W, G_R)
    T_t = np.einsum("vj,fja->fva", W, A_t)
    verts = np.einsum("fvab,fvb->fva", T_R, v_posed) + T_t + trans[:, None, :]
    return verts, G_t + trans[:, None, :], T_R


def rest_joints_f64(tables: SmplTables, betas: np.ndarray) -> np.ndarray:
    """Rest joints [24,3] of the shape `betas` [10], float64."""
    Jr = tables.J_regressor.astype(np.float64)
    v = tables.v_template.astype(np.float64) + tables.shapedirs.astype(np.float64) @ np.asarray(betas, dtype=np.float64).reshape(10)
    return Jr @ v


def fk_joints_f64(tables: SmplTables, rot: np.ndarray, rest: np.ndarray):
    """The kinematic chain of lbs_f64 alone on rest joints `rest` [24,3] (rest_joints_f64): joints [F,24,3] at zero translation
    and world rotations [F,24,3,3]."""
    F = rot.shape[0]
    J = np.broadcast_to(rest[None], (F, NUM_JOINTS, 3))
    G_R = np.zeros((F, NUM_JOINTS, 3, 3))
    G_t = np.zeros((F, NUM_JOINTS, 3))
    G_R[:, 0] = rot[:, 0]
    G_t[:, 0] = J[:, 0]
    for j in range(1, NUM_JOINTS):
        p = tables.parents[j]
        G_R[:, j] = G_R[:, p] @ rot[:, j]
        G_t[:, j] = np.einsum("fab,fb->fa", G_R[:, p], J[:, j] - J[:, p]) + G_t[:, p]
    return G_t, G_R


#: the elbow capture (make_sequence(elbow_error=True)): window length, the forearm's turn about the camera's depth axis, taper
ELBOW_WINDOW, ELBOW_ANGLE, ELBOW_TAPER = 24, 0.5, 2
OUTLIER_WINDOW, OUTLIER_ANGLE, OUTLIER_TAPER = 24, 1.0, 2  # make_sequence(pose_outlier=True): the left hip's twist


#: the self-penetration capture (make_sequence(self_penetration=True)): window length, depth of the HMR start's overlap, taper
PENETRATION_WINDOW, PENETRATION_DEPTH, PENETRATION_TAPER = 24, 0.030, 2


def _arm_into_torso(tables, hmr_rot, rest, caps, t0):
    """The HMR stand-in's left shoulder (joint 16) in frames t0 .. t0 + 23, rotated in the world frame about the axis
    (arm direction) x (direction from the shoulder to the spine line, pelvis -> neck) by the angle at which the deepest overlap of
    the left arm's capsules (joints 16, 18, 20, 22) with the trunk's (joints 0, 3, 6, 9, 12) -- over the pairs of the default list,
    on the rest joints `rest` -- is PENETRATION_DEPTH; the angle is the first crossing on a grid of pi / 64, refined by 40 bisections, and tapered
    (1/3, 2/3) over two frames at each end.  Returns the changed copy of hmr_rot and the indices of the arm / trunk pairs."""
    from .body_model import capsule_pair_depths

    cj, cg, pr = caps
    arm = np.isin(cj, [16, 18, 20, 22]).all(axis=1)
    trunk = np.isin(cj, [0, 3, 6, 9, 12]).all(axis=1)
    sel = np.array([k for k, (i, j) in enumerate(pr) if (arm[i] and trunk[j]) or (arm[j] and trunk[i])], dtype=np.int64)
    if len(sel) == 0:
        raise ValueError("make_sequence: the default capsule list has no arm / trunk pair")
    out = hmr_rot.copy()
    n = PENETRATION_WINDOW
    for i in range(n):
        f = t0 + i
        rot_f = hmr_rot[f:f + 1]
        J, G = fk_joints_f64(tables, rot_f, rest)
        d_arm = J[0, 18] - J[0, 16]
        d_arm /= np.linalg.norm(d_arm)
        e = J[0, 12] - J[0, 0]
        foot = J[0, 0] + ((J[0, 16] - J[0, 0]) @ e) / (e @ e) * e
        axis = np.cross(d_arm, foot - J[0, 16])
        axis /= np.linalg.norm(axis)
        G13 = G[0, 13]

        def posed(theta):
            r = rot_f.copy()
            r[0, 16] = G13.T @ _rodrigues(theta * axis) @ G13 @ rot_f[0, 16]
            return r

        def depth(theta):
            return capsule_pair_depths(fk_joints_f64(tables, posed(theta), rest)[0], cj, cg, pr[sel]).max()

        grid = np.linspace(0.0, np.pi, 65)
        hi = next((th for th in grid[1:] if depth(th) >= PENETRATION_DEPTH), None)
        if hi is None:
            raise ValueError("make_sequence: frame %d: no shoulder angle puts the left arm %.0f mm into the trunk"
                             % (f, 1e3 * PENETRATION_DEPTH))
        lo = hi - np.pi / 64.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if depth(mid) >= PENETRATION_DEPTH:
                hi = mid
            else:
                lo = mid
        edge = min(i, n - 1 - i)
        taper = 1.0 if edge >= PENETRATION_TAPER else (edge + 1.0) / (PENETRATION_TAPER + 1.0)
        out[f, 16] = posed(taper * hi)[0, 16]
    return out, sel


#: the joint-limit capture (make_sequence(joint_limits=True)): the limited (joint, component, allowed direction) of the true motion,
#: window length, the x component of the HMR start's left knee there (radians), taper
LIMITED_COMPONENTS = ((4, 0, 1.0), (5, 0, 1.0), (18, 1, -1.0), (19, 1, 1.0))
LIMIT_WINDOW, LIMIT_KNEE_X, LIMIT_TAPER = 24, -0.5, 2
#: video_dropout: frames for which the video loses the person (three seconds at 30 Hz)
DROPOUT_WINDOW = 90


def farthest_point_vertices(points: np.ndarray, count: int, start: int = 0) -> np.ndarray:
    chosen = [int(start)]
    d = np.linalg.norm(points - points[start], axis=1)
    for _ in range(count - 1):
        nxt = int(np.argmax(d))
        chosen.append(nxt)
        d = np.minimum(d, np.linalg.norm(points - points[nxt], axis=1))
    return np.array(chosen, dtype=np.int64)


class SyntheticMarkers:
    """``Markers`` duck-type (reference markers/markers.py:35-54)."""

    def __init__(self, points: np.ndarray, freq: float = 30.0):
        self._points = points
        self._freq = freq

    def get_points(self):
        return self._points

    def set_points(self, points):
        self._points = points

    def get_frequency(self):
        return self._freq


@dataclass
class SyntheticImgSmpl:
    """``ImgSmpl`` duck-type: the fields multimodal_video_mocap reads (reference multimodal.py:88-100)."""

    trans: torch.Tensor
    root_orient: torch.Tensor
    hmr_root_orient: torch.Tensor
    pose_body: torch.Tensor
    betas: torch.Tensor
    foot_contacts: torch.Tensor
    camera_bbox: torch.Tensor
    center: torch.Tensor
    scale: torch.Tensor
    size: torch.Tensor
    img_mask: torch.Tensor
    freq: float = 30.0


@dataclass
class SyntheticSequence:
    img_smpl: SyntheticImgSmpl
    markers: SyntheticMarkers
    gt: dict


def _motion_axis_angles(seed: int, F: int):
    """The ground-truth motion of make_sequence(seed, num_frames=F): the joints' axis-angle vectors [F, 24, 3] (the root's row is
    zero: make_sequence builds the root's rotation apart) with their amplitudes, frequencies and phases [24, 3]."""
    s = 7919 * (seed + 1)
    t = np.arange(F, dtype=np.float64) / max(F, 1)
    amp = 0.6 * hash_uniform(s + 1, NUM_JOINTS, 3)
    amp[0] = 0.0
    amp[[10, 11, 22, 23]] *= 0.3  # feet / hands move less
    freq = 0.5 + 2.5 * hash_uniform(s + 2, NUM_JOINTS, 3)
    phase = 2.0 * np.pi * hash_uniform(s + 3, NUM_JOINTS, 3)
    aa = amp[None] * np.sin(2.0 * np.pi * freq[None] * t[:, None, None] + phase[None])  # [F,24,3]
    return aa, amp, freq, phase


_POSE_MIXTURES = {}


def pose_mixture(K: int = 8, seeds=range(100, 132), num_frames: int = 64):
    """EXTENSION: a deterministic stand-in for a learned pose mixture (no learned one, SMPLify's gmm_08, is at hand):
    {"means" [K, 69], "covars" [K, 69, 69], "weights" [K]} in float64 from the ground-truth body poses of
    make_sequence(seed, num_frames=num_frames) at `seeds`, which the tests and the bench do not fit.  numpy only: theta [N, 69]
    the axis-angle vectors of joints 1 .. 23, k-means with 20 Lloyd iterations from the start centres theta[i N // K] (an empty
    cluster keeps its centre), then per cluster the mean, the covariance (about the mean, / n) plus 1e-3 rad^2 on the
    diagonal, and the share of the samples as weight; a cluster left empty takes its centre, the diagonal alone and the weight
    of one sample.  The motion's components are independent sines: the mixture can show the pull on an outlier, not the value
    of a learned mixture's correlations."""
    key = (int(K), tuple(int(q) for q in seeds), int(num_frames))
    if key in _POSE_MIXTURES:
        return {k: v.copy() for k, v in _POSE_MIXTURES[key].items()}
    K = key[0]
    if not 1 <= K <= 16:
        raise ValueError("pose_mixture: 1 .. 16 components (got %d)" % K)
    theta = np.concatenate([_motion_axis_angles(q, key[2])[0][:, 1:].reshape(key[2], 69) for q in key[1]], axis=0)
    N = theta.shape[0]
    if N < K:
        raise ValueError("pose_mixture: %d poses are fewer than the %d components" % (N, K))
    centres = theta[[(i * N) // K for i in range(K)]].copy()
    for _ in range(20):
        label = np.argmin(((theta[:, None, :] - centres[None]) ** 2).sum(-1), axis=1)
        for k in range(K):
            if (label == k).any():
                centres[k] = theta[label == k].mean(axis=0)
    label = np.argmin(((theta[:, None, :] - centres[None]) ** 2).sum(-1), axis=1)
    means, covars, weights = centres.copy(), np.zeros((K, 69, 69)), np.zeros(K)
    for k in range(K):
        x = theta[label == k]
        weights[k] = max(len(x), 1) / float(N)
        if len(x):
            means[k] = x.mean(axis=0)
            d = x - means[k][None]
            covars[k] = d.T @ d / len(x)
        covars[k] += 1e-3 * np.eye(69)
    out = {"means": means, "covars": covars, "weights": weights / weights.sum()}
    _POSE_MIXTURES[key] = {k: v.copy() for k, v in out.items()}
    return out


def make_sequence(tables: SmplTables, seed: int = 0, num_frames: int = 300, num_markers: int = 50,
                  limb_only: bool = False, yaw_offset_deg: float = 100.0, dropout: float = 0.02,
                  hmr_pose_noise: float = 0.1, hmr_beta_noise: float = 0.5, subject_seed: int = None,
                  standoff_tilt_deg: float = 0.0, standoff_mm=(9.5, 9.5), planted_feet: bool = False,
                  stance_frames: int = 20, identity_events: int = 0, floor: bool = False,
                  self_penetration: bool = False, joint_limits: bool = False,
                  video_dropout: bool = False, elbow_error: bool = False, pose_outlier: bool = False) -> SyntheticSequence:
    """One synthetic sequence: smooth GT motion, unlabeled-but-tracked markers 9.5 mm off the
    surface with 1 mm noise and block dropout, and an HMR stand-in (noisy pose/shape, wrong yaw).  `subject_seed` fixes the
    ground-truth shape independently of `seed`: sequences of ONE subject (the shared-betas extension fits them together).
    Marker m sits at its vertex + T_R o_m, o_m a rest-space offset skinned with the vertex's blended rotation; by default
    o_m = 9.5 mm along the outward direction.  A stand-off capture (EXTENSION tests of the latent marker offsets):
    `standoff_tilt_deg` > 0 tilts every direction off the outward one by up to that angle about a random axis, and
    `standoff_mm` = (lo, hi) draws every length uniformly from [lo, hi] mm.  gt["marker_offsets"] holds the o_m [M, 3]
    (metres, column order).
    A planted-feet capture (EXTENSION tests of the foot-lock term): with `planted_feet` the pose track is unchanged and the
    translation is rebuilt so that the stance foot's joint (10 left, 11 right; foot (t // stance_frames) % 2) does not move:
    trans_t = trans_{t-1} - (j_t[foot] - j_{t-1}[foot]) with j the joints at zero translation.  gt["foot_contacts"] [F, 2] holds
    the true stance labels; img_smpl.foot_contacts the same eroded by two frames at each end of every stance (a detector that
    is late and early, never wrong).
    A capture with a floor (EXTENSION tests of the floor-contact term): `floor` (with `planted_feet`; ValueError without) keeps
    the planted translation in x and y and sets trans_z[t] so that the lowest of the body_model.sole_vertices points, over both
    feet, lies exactly at z = 0 in every frame (float64).  gt["foot_contacts"][t, s] is then 1 only where foot s is the stance
    foot AND its lowest sole point is within 5 mm of the floor; img_smpl.foot_contacts is that array eroded by two frames at each
    end of every run.  gt["sole_vids"] [2, 3] are the points, gt["floor_height"] = 0.0, gt["sole_z"] [F, 6] their float64
    heights (left foot first).  No hash stream is consumed; without the option every array is what it was.
    A capture whose video start penetrates itself (EXTENSION tests of the self-penetration term): `self_penetration` picks a
    window of 24 frames -- the first run starting at or after F / 10 in which the ground truth has zero overlap in every pair of
    body_model.body_capsules (float64; ValueError if there is none) --, rotates the HMR stand-in's left shoulder there until the
    arm's capsules sit 30 mm inside the trunk's (_arm_into_torso; the angle tapered over two frames at each end), and blanks
    (exact zeros) every marker column owned by joints 16, 18, 20, 22 in the window.  gt["capsules"] is the capsule list,
    gt["penetration_window"] = (first frame, one past the last), gt["hmr_overlap"] [F] the HMR start's deepest arm / trunk overlap
    per frame (metres, at its mean betas).  No hash stream is consumed; without the option every array is what it was.
    A capture whose video start bends a knee backwards (EXTENSION tests of the joint-angle limit term): with `joint_limits` the
    ground truth's four limited components (LIMITED_COMPONENTS: knees x, elbows y) become d |A| (1 + sin(2 pi f t + phi)) with
    A, f, phi the component's own and d the allowed direction, so that the true motion lies inside body_model.smpl_joint_limits()
    in every frame.  In a window of 24 frames starting at F / 10 (rounded up; ValueError if the sequence is shorter) the x
    component of the axis-angle vector of the HMR stand-in's left knee (joint 4) is replaced by -0.5 rad, about 29 degrees
    backwards (tapered 1/3, 2/3 over two frames at each end), and every marker column owned by joints 4, 7 and 10 is blanked
    (exact zeros): nothing but the prior then holds the shank.  gt["joint_limits"] = (lo, hi) are the default tables,
    gt["limit_window"] = (first frame, one past the last), gt["hmr_violation"] [F] the HMR start's largest violation per frame
    (radians).  No hash stream is consumed; without the option every array is what it was.
    A capture whose columns change identity (EXTENSION tests of the tracklet placement): `identity_events` events, each at a
    frame t_e in [F/10, 9F/10) and on three columns visible at t_e whose mutual distances there are >= 0.2 m (frame and columns
    from the event's own hash stream, drawn again until they qualify).  From t_e on the contents of the three columns are
    rotated cyclically (a takes b's, b takes c's, c takes a's); every second event also blanks the three columns for the five
    frames before t_e.  gt["marker_vids_fm"] [F, M] holds the true vertex of every entry (-1 where missing), gt["tracklets_fm"]
    [F, M] the true tracklet ids (a run of consecutive visible frames of one column showing one marker; dense ids ordered by
    (column, start), -1 where missing).  With 0 events no hash stream is consumed and every other array is unchanged.
    A capture whose video loses the person (EXTENSION tests of the pose prior's weights): with `video_dropout` the tracker drops
    the subject for DROPOUT_WINDOW = 90 frames from frame F / 3 on (rounded up; ValueError unless a seen frame is left on both
    sides).  img_mask is False there, and the stand-in's pose_body, root_orient, hmr_root_orient, trans and betas in the window
    are what ingest.fill_gaps makes of its own neighbours (slerp / lerp across the gap), as ingest.ImgSmpl would; foot_contacts
    are 0 there.  The markers are untouched.  gt["dropout_window"] = (first frame, one past the last), gt["hmr_gap_error"] [F]
    the mean geodesic distance (radians, over the 23 body joints) of the stand-in's pose -- filled, inside the window -- from
    the ground truth's.  No hash stream is consumed; without the option every array is what it was.
    A capture whose video start has an elbow wrong in the image plane (EXTENSION tests of the 2D key-point term): with
    `elbow_error`, in a window of ELBOW_WINDOW = 24 frames starting at F / 10 (rounded up; ValueError if the sequence is shorter)
    the HMR stand-in's left forearm (joint 18, the elbow) is turned by ELBOW_ANGLE = 0.5 rad about the world y axis -- the depth
    direction of synthetic_camera, so the error lies in its image plane -- (tapered 1/3, 2/3 over two frames at each end), and
    every marker column owned by joints 16, 18, 20 and 22 is blanked (exact zeros): nothing but the prior then holds the arm.
    gt["elbow_window"] = (first frame, one past the last).  No hash stream is consumed; without the option every array is what
    it was.
    A capture whose video start twists a hip (EXTENSION tests of the mixture pose prior): with `pose_outlier`, in a window of
    OUTLIER_WINDOW = 24 frames starting at F / 10 (rounded up; ValueError if the sequence is shorter) the HMR stand-in's left hip
    (joint 1) is turned by OUTLIER_ANGLE = 1.0 rad about its own y axis -- twist about the thigh, which no hinge limit, capsule or
    smoothness term prices -- (tapered 1/3, 2/3 over two frames at each end), and every marker column owned by joints 1, 4, 7 and
    10 is blanked (exact zeros): nothing but the prior then holds the leg.  gt["outlier_window"] = (first frame, one past the
    last), gt["hmr_outlier_error"] [F] the geodesic distance (radians) of the stand-in's joint 1 from the truth.  No hash stream
    is consumed; without the option every array is what it was."""
    F, M = num_frames, num_markers
    if floor and not planted_feet:
        raise ValueError("make_sequence: floor=True needs planted_feet=True (the floor is built under the planted feet)")
    s = 7919 * (seed + 1)
    t = np.arange(F, dtype=np.float64) / max(F, 1)

    # --- ground-truth motion
    aa, amp, freq, phase = _motion_axis_angles(seed, F)
    if joint_limits:  # (no hash stream: the four limited components of the true motion stay on the allowed side)
        for jj, kk, dd in LIMITED_COMPONENTS:
            aa[:, jj, kk] = dd * np.abs(amp[jj, kk]) * (1.0 + np.sin(2.0 * np.pi * freq[jj, kk] * t + phase[jj, kk]))
    rot = _rodrigues(aa)
    yaw = 1.0 * np.sin(2.0 * np.pi * 0.5 * t + 2.0 * np.pi * hash_uniform(s + 4))
    up = _rodrigues(np.array([np.pi / 2.0, 0.0, 0.0]))  # SMPL y-up -> mocap z-up
    wobble = _rodrigues(0.15 * np.sin(2.0 * np.pi * t[:, None] * np.array([1.0, 1.5, 0.7])[None]
                                      + 2.0 * np.pi * hash_uniform(s + 5, 3)[None]))
    Rz = _rodrigues(np.stack([np.zeros(F), np.zeros(F), yaw], axis=-1))
    rot[:, 0] = Rz @ up[None] @ wobble
    steps = hash_normal(s + 6, F, 3) * 0.02
    walk = np.cumsum(steps, axis=0)
    k = np.exp(-0.5 * (np.arange(-15, 16) / 5.0) ** 2)
    k /= k.sum()
    walk = np.stack([np.convolve(np.pad(walk[:, a], 15, mode="edge"), k, mode="valid") for a in range(3)], axis=1)
    walk = np.clip(walk, -1.0, 1.0)
    trans = walk + np.array([0.0, 0.0, 0.95])[None]
    beta_gt = np.clip(hash_normal((s if subject_seed is None else 7919 * (int(subject_seed) + 1)) + 7, 10), -2.0, 2.0)[None]

    contacts_gt = contacts_seen = sole = sole_z = None
    if planted_feet:  # (no hash stream: every other array is made from the rebuilt translation exactly as without the option)
        stance_frames = int(stance_frames)
        if stance_frames < 1:
            raise ValueError("make_sequence: stance_frames must be at least 1")
        v0, j0, _ = lbs_f64(tables, rot, beta_gt, np.zeros((F, 3)))
        stance = (np.arange(F) // stance_frames) % 2
        for i in range(1, F):
            foot = 10 + stance[i]
            trans[i] = trans[i - 1] - (j0[i, foot] - j0[i - 1, foot])
        contacts_gt = np.zeros((F, 2))
        contacts_gt[np.arange(F), stance] = 1.0
        contacts_seen = np.zeros((F, 2))
        for a0 in range(0, F, stance_frames):
            b0 = min(a0 + stance_frames, F)
            contacts_seen[a0 + 2:max(b0 - 2, a0 + 2), stance[a0]] = 1.0
        if floor:  # the lowest sole point of every frame on z = 0; contacts only where the stance foot really is down
            from .body_model import sole_vertices

            sole = sole_vertices(tables)
            z0 = v0[:, sole.reshape(-1), 2]
            trans[:, 2] = -z0.min(axis=1)
            sole_z = z0 + trans[:, 2:3]
            k = sole.shape[1]
            low = np.stack([sole_z[:, :k].min(axis=1), sole_z[:, k:].min(axis=1)], axis=1)
            contacts_gt = contacts_gt * (low <= 0.005)
            contacts_seen = np.zeros((F, 2))
            for sft in range(2):
                on = np.concatenate([[0.0], contacts_gt[:, sft], [0.0]])
                starts, ends = np.where(np.diff(on) > 0)[0], np.where(np.diff(on) < 0)[0]
                for a0, b0 in zip(starts, ends):
                    contacts_seen[a0 + 2:max(b0 - 2, a0 + 2), sft] = 1.0
        del v0

    verts, joints, T_R = lbs_f64(tables, rot, beta_gt, trans)

    # --- markers: farthest-point vertex ids, 9.5 mm outward, 1 mm noise
    vt = tables.v_template.astype(np.float64)
    owner = np.argmax(tables.lbs_weights, axis=1)
    if limb_only:
        cand = np.where(np.isin(owner, [16, 18, 20, 22]))[0]  # left arm
    else:
        cand = np.arange(vt.shape[0])
    pick = cand[farthest_point_vertices(vt[cand], M, start=int(hash_uniform(s + 8) * len(cand)))]
    J0 = tables.J_regressor.astype(np.float64) @ vt
    ends = J0.copy()
    for j in range(NUM_JOINTS):
        kids = np.where(tables.parents == j)[0]
        ends[j] = J0[kids].mean(axis=0) if len(kids) else J0[j] + (J0[j] - J0[tables.parents[j]])
    a = J0[owner[pick]]
    b = ends[owner[pick]]
    ab = b - a
    tt = np.clip(np.sum((vt[pick] - a) * ab, axis=1) / np.maximum(np.sum(ab * ab, axis=1), 1e-12), 0.0, 1.0)
    out_dir = vt[pick] - (a + tt[:, None] * ab)
    out_dir /= np.maximum(np.linalg.norm(out_dir, axis=1, keepdims=True), 1e-9)
    out_world = np.einsum("fmab,mb->fma", T_R[:, pick], out_dir)
    if standoff_tilt_deg == 0.0 and tuple(standoff_mm) == (9.5, 9.5):
        offsets = 0.0095 * out_dir
        markers = verts[:, pick] + 0.0095 * out_world + 0.001 * hash_normal(s + 9, F, M, 3)
    else:  # stand-off capture: tilted directions, per-marker lengths (own hash streams: the other arrays do not change)
        r = hash_normal(s + 15, M, 3)
        perp = r - np.sum(r * out_dir, axis=1, keepdims=True) * out_dir
        perp /= np.maximum(np.linalg.norm(perp, axis=1, keepdims=True), 1e-9)
        ang = np.deg2rad(float(standoff_tilt_deg)) * hash_uniform(s + 16, M)
        dirs = np.cos(ang)[:, None] * out_dir + np.sin(ang)[:, None] * perp
        lo, hi = (float(v) * 1e-3 for v in standoff_mm)
        offsets = (lo + (hi - lo) * hash_uniform(s + 17, M))[:, None] * dirs
        markers = verts[:, pick] + np.einsum("fmab,mb->fma", T_R[:, pick], offsets) + 0.001 * hash_normal(s + 9, F, M, 3)
    perm = np.argsort(hash_uniform(s + 10, M), kind="stable")
    markers = markers[:, perm]
    # block dropout: (marker, 10-frame block) zeroed (style of reference markers/markers_noise.py:39-66)
    nblocks = (F + 9) // 10
    drop = hash_uniform(s + 11, nblocks, M) < dropout
    drop_f = np.repeat(drop, 10, axis=0)[:F]
    markers = np.where(drop_f[..., None], 0.0, markers)
    # identity events (own hash streams; none consumed with 0 events): which physical marker (index into pick[perm]) a column shows
    identity = np.broadcast_to(np.arange(M)[None, :], (F, M)).copy()
    identity_events = int(identity_events)
    if identity_events < 0 or (identity_events > 0 and (M < 3 or F < 10)):
        raise ValueError("make_sequence: identity_events needs a count >= 0, at least 3 markers and 10 frames")
    for e in range(identity_events):
        draws = hash_uniform(s + 1000 + e, 256, 4)
        for u in draws:
            fe = int(F // 10 + u[0] * (9 * F // 10 - F // 10))
            cols = [int(u[1 + i] * M) for i in range(3)]
            if len(set(cols)) < 3:
                continue
            x = markers[fe, cols]
            if not np.all(np.abs(x).sum(axis=1) != 0.0):
                continue
            if min(np.linalg.norm(x[i] - x[j]) for i, j in ((0, 1), (0, 2), (1, 2))) < 0.2:
                continue
            break
        else:
            raise ValueError("make_sequence: no three columns 0.2 m apart found for identity event %d" % e)
        src = [cols[1], cols[2], cols[0]]
        markers[fe:, cols] = markers[fe:, src]
        identity[fe:, cols] = identity[fe:, src]
        if e % 2 == 1:
            markers[max(fe - 5, 0):fe, cols] = 0.0
    visible = np.abs(markers).sum(axis=-1) != 0.0
    vids_fm = np.where(visible, pick[perm][identity], -1)
    from .tracklets import tracklets_from_identity

    tracklets_fm = tracklets_from_identity(torch.from_numpy(np.where(visible, identity, -1))).seg.numpy()

    # --- HMR stand-in
    noise_aa = hmr_pose_noise * hash_normal(s + 12, F, NUM_JOINTS, 3)
    hmr_rot = rot @ _rodrigues(noise_aa)
    yaw_off = _rodrigues(np.array([0.0, 0.0, np.deg2rad(yaw_offset_deg)]))
    hmr_root = yaw_off[None] @ hmr_rot[:, 0]
    hmr_betas = beta_gt + hmr_beta_noise * hash_normal(s + 13, F, 10)
    hmr_trans = trans + 0.05 * hash_normal(s + 14, F, 3)

    caps = window = hmr_overlap = None
    if self_penetration:  # (no hash stream: the HMR pose of the window and the arm's marker columns there change, nothing else)
        from .body_model import body_capsules, capsule_pair_depths

        caps = body_capsules(tables)
        free = capsule_pair_depths(joints, *caps).max(axis=1) == 0.0
        start = -(-F // 10)
        t0 = next((a0 for a0 in range(start, F - PENETRATION_WINDOW + 1) if free[a0:a0 + PENETRATION_WINDOW].all()), None)
        if t0 is None:
            raise ValueError("make_sequence: no window of %d frames from frame %d on in which the ground truth is free of "
                             "overlap" % (PENETRATION_WINDOW, start))
        window = (t0, t0 + PENETRATION_WINDOW)
        rest = rest_joints_f64(tables, hmr_betas.mean(axis=0))  # (the fit starts from the mean of the HMR betas)
        hmr_rot, sel = _arm_into_torso(tables, hmr_rot, rest, caps, t0)
        hmr_overlap = capsule_pair_depths(fk_joints_f64(tables, hmr_rot, rest)[0], caps[0], caps[1], caps[2][sel]).max(axis=1)
        arm_cols = np.isin(owner[pick[perm]], [16, 18, 20, 22])
        markers[t0:t0 + PENETRATION_WINDOW, arm_cols] = 0.0

    limits = limit_window = hmr_violation = None
    if joint_limits:  # (no hash stream: the HMR knee of the window and the left leg's marker columns there change, nothing else)
        from .body_model import joint_limit_violation, rotation_log, smpl_joint_limits

        t0 = -(-F // 10)
        if t0 + LIMIT_WINDOW > F:
            raise ValueError("make_sequence: joint_limits needs a window of %d frames from frame %d on (F = %d)" % (LIMIT_WINDOW, t0, F))
        limits = smpl_joint_limits()
        limit_window = (t0, t0 + LIMIT_WINDOW)
        hmr_rot = hmr_rot.copy()
        for i in range(LIMIT_WINDOW):
            edge = min(i, LIMIT_WINDOW - 1 - i)
            taper = 1.0 if edge >= LIMIT_TAPER else (edge + 1.0) / (LIMIT_TAPER + 1.0)
            om = rotation_log(hmr_rot[t0 + i, 4])[0]
            om[0] = taper * LIMIT_KNEE_X
            hmr_rot[t0 + i, 4] = _rodrigues(om)
        hmr_violation = joint_limit_violation(hmr_rot[:, 1:], *limits).reshape(F, -1).max(axis=1)
        leg_cols = np.isin(owner[pick[perm]], [4, 7, 10])
        markers[t0:t0 + LIMIT_WINDOW, leg_cols] = 0.0

    elbow_window = None
    if elbow_error:  # (no hash stream: the HMR elbow of the window and the left arm's marker columns there change, nothing else)
        t0 = -(-F // 10)
        if t0 + ELBOW_WINDOW > F:
            raise ValueError("make_sequence: elbow_error needs a window of %d frames from frame %d on (F = %d)" % (ELBOW_WINDOW, t0, F))
        elbow_window = (t0, t0 + ELBOW_WINDOW)
        hmr_rot = hmr_rot.copy()
        world = fk_joints_f64(tables, hmr_rot, rest_joints_f64(tables, hmr_betas.mean(axis=0)))[1][:, 18]
        for i in range(ELBOW_WINDOW):
            edge = min(i, ELBOW_WINDOW - 1 - i)
            taper = 1.0 if edge >= ELBOW_TAPER else (edge + 1.0) / (ELBOW_TAPER + 1.0)
            axis_local = world[t0 + i].T @ np.array([0.0, 1.0, 0.0])   # a turn about world y, said in the forearm's own frame
            hmr_rot[t0 + i, 18] = hmr_rot[t0 + i, 18] @ _rodrigues(taper * ELBOW_ANGLE * axis_local)
        arm_cols = np.isin(owner[pick[perm]], [16, 18, 20, 22])
        markers[t0:t0 + ELBOW_WINDOW, arm_cols] = 0.0

    outlier_window = hmr_outlier_error = None
    if pose_outlier:  # (no hash stream: the HMR hip of the window and the left leg's marker columns there change, nothing else)
        t0 = -(-F // 10)
        if t0 + OUTLIER_WINDOW > F:
            raise ValueError("make_sequence: pose_outlier needs a window of %d frames from frame %d on (F = %d)" % (OUTLIER_WINDOW, t0, F))
        outlier_window = (t0, t0 + OUTLIER_WINDOW)
        hmr_rot = hmr_rot.copy()
        for i in range(OUTLIER_WINDOW):
            edge = min(i, OUTLIER_WINDOW - 1 - i)
            taper = 1.0 if edge >= OUTLIER_TAPER else (edge + 1.0) / (OUTLIER_TAPER + 1.0)
            hmr_rot[t0 + i, 1] = hmr_rot[t0 + i, 1] @ _rodrigues(np.array([0.0, taper * OUTLIER_ANGLE, 0.0]))
        rel = np.einsum("fab,fac->fbc", rot[:, 1], hmr_rot[:, 1])
        hmr_outlier_error = np.arccos(np.clip(0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0), -1.0, 1.0))
        leg_cols = np.isin(owner[pick[perm]], [1, 4, 7, 10])
        markers[t0:t0 + OUTLIER_WINDOW, leg_cols] = 0.0

    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    img_mask = torch.ones(F, dtype=torch.bool)
    tracks = {"trans": f32(hmr_trans), "root_orient": f32(hmr_root[:, None]), "pose_body": f32(hmr_rot[:, 1:]),
              "betas": f32(hmr_betas)}
    contacts_img = f32(contacts_seen) if planted_feet else torch.zeros(F, 2)
    dropout_window = hmr_gap_error = None
    if video_dropout:  # (no hash stream: the video's tracks and labels inside the window change, nothing else)
        from .ingest import fill_gaps

        t0 = -(-F // 3)
        if t0 < 1 or t0 + DROPOUT_WINDOW >= F:
            raise ValueError("make_sequence: video_dropout needs a window of %d frames from frame %d on with a seen frame on both "
                             "sides (F = %d)" % (DROPOUT_WINDOW, t0, F))
        dropout_window = (t0, t0 + DROPOUT_WINDOW)
        img_mask[t0:t0 + DROPOUT_WINDOW] = False
        tracks = fill_gaps(tracks, img_mask)
        contacts_img = contacts_img.clone()
        contacts_img[t0:t0 + DROPOUT_WINDOW] = 0.0
        rel = np.einsum("fjab,fjac->fjbc", rot[:, 1:], tracks["pose_body"].numpy().astype(np.float64))
        cos = np.clip(0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0), -1.0, 1.0)
        hmr_gap_error = np.arccos(cos).mean(axis=1)
    img = SyntheticImgSmpl(
        trans=tracks["trans"],
        root_orient=tracks["root_orient"],
        hmr_root_orient=tracks["root_orient"].clone(),
        pose_body=tracks["pose_body"],
        betas=tracks["betas"],
        foot_contacts=contacts_img,
        camera_bbox=torch.zeros(F, 3),
        center=torch.zeros(F, 2),
        scale=torch.zeros(F, 1),
        size=torch.zeros(F, 2),
        img_mask=img_mask,
        freq=30.0,
    )
    gt = {
        "rot": rot.astype(np.float32), "betas": beta_gt.astype(np.float32), "trans": trans.astype(np.float32),
        "verts": verts.astype(np.float32), "joints": joints.astype(np.float32),
        "marker_vids": pick[perm],
        "marker_offsets": offsets[perm].astype(np.float32),
        "marker_vids_fm": vids_fm.astype(np.int64), "tracklets_fm": tracklets_fm.astype(np.int32),
    }
    if planted_feet:
        gt["foot_contacts"] = contacts_gt.astype(np.float32)
    if floor:
        gt["sole_vids"] = sole
        gt["floor_height"] = 0.0
        gt["sole_z"] = sole_z
    if self_penetration:
        gt["capsules"] = caps
        gt["penetration_window"] = window
        gt["hmr_overlap"] = hmr_overlap
    if joint_limits:
        gt["joint_limits"] = limits
        gt["limit_window"] = limit_window
        gt["hmr_violation"] = hmr_violation
    if video_dropout:
        gt["dropout_window"] = dropout_window
        gt["hmr_gap_error"] = hmr_gap_error
    if elbow_error:
        gt["elbow_window"] = elbow_window
    if pose_outlier:
        gt["outlier_window"] = outlier_window
        gt["hmr_outlier_error"] = hmr_outlier_error
    return SyntheticSequence(img_smpl=img, markers=SyntheticMarkers(markers.astype(np.float32), 30.0), gt=gt)


def synthetic_hmr_camera(num_frames: int, seed: int = 5):
    """A plausible HMR 2.0 weak-perspective camera for the reprojection stage: `camera_bbox` (scale, shift x, shift y)
    [F,3], bounding-box `center` [F,2] in pixels, image `size` (H, W) [F,2] and bounding-box `scale` [F,1]."""
    from .body_model import hash_uniform

    u = hash_uniform(seed, num_frames, 6)
    pred_cam = np.stack([0.85 + 0.2 * u[:, 0], 0.1 * (u[:, 1] - 0.5), 0.1 * (u[:, 2] - 0.5)], axis=1)
    center = np.stack([300.0 + 40 * u[:, 3], 220.0 + 30 * u[:, 4]], axis=1)
    size = np.tile(np.array([[480.0, 640.0]]), (num_frames, 1))
    scale = 0.35 + 0.1 * u[:, [5]]
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (pred_cam, center, size, scale)]


def synthetic_camera(seq: SyntheticSequence, distance: float = 4.0, focal: float = 1000.0, centre=(960.0, 540.0)) -> np.ndarray:
    """A fixed pinhole camera for a z-up capture, as one row of 16 floats (A 3x3 row-major, b, fx, fy, cx, cy; p = A J + b):
    it stands `distance` metres in front of the mean ground-truth joint and looks along world +y; image x is world x, image y is
    world -z.  Pixels."""
    A = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    mean = np.asarray(seq.gt["joints"], dtype=np.float64)[:, :24].reshape(-1, 3).mean(axis=0)
    b = np.array([0.0, 0.0, float(distance)]) - A @ mean
    return np.concatenate([A.reshape(-1), b, [float(focal), float(focal), float(centre[0]), float(centre[1])]])


def synthetic_keypoints_2d(seq: SyntheticSequence, camera=None, noise: float = 2.0, seed: int = 0, dropped_frames=()):
    """EXTENSION: the `keypoints_2d` record of a synthetic capture (terms.check_keypoints_2d) -- the 24 ground-truth kinematic
    joints projected through one fixed camera (`camera`: 16 floats, default synthetic_camera(seq)), plus Gaussian noise of
    `noise` units (pixels) per coordinate from the hash stream of `seed`; confidence 1, and 0 in every frame of
    `dropped_frames` (a detector that lost the person).  Targets made from the ground truth: what a perfect calibration and an
    unbiased detector would give."""
    from .body_model import hash_normal

    J = np.asarray(seq.gt["joints"], dtype=np.float64)[:, :24]
    F = J.shape[0]
    cam = np.asarray(synthetic_camera(seq) if camera is None else camera, dtype=np.float64).reshape(16)
    p = J @ cam[:9].reshape(3, 3).T + cam[9:12]
    u = np.stack([cam[12] * p[..., 0] / p[..., 2] + cam[14], cam[13] * p[..., 1] / p[..., 2] + cam[15]], axis=-1)
    u = u + float(noise) * hash_normal(104729 * (int(seed) + 1), F, 24, 2)
    conf = np.ones((F, 24))
    conf[list(dropped_frames)] = 0.0
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return {"camera": f32(np.tile(cam[None], (F, 1))), "targets": f32(u), "confidence": f32(conf)}
