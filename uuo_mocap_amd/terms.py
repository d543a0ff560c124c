"""The EXTENSION terms of the chamfer and marker stages, once: their config parsers, one table row per term (TERMS) with
everything the host layer knows about it -- loss keys and stages, the `execution.*` switch, what a lock-step batch, frame-block
sharding, the fused soft-assignment closure and the per-frame vertex table make of it (with the refusal texts), its term on the
closures composed from the operators, and how its state on a stage problem is armed on a workspace -- the sets of allowed loss
keys derived from the rows, and the one decision which closure a stage runs on (stage_route, lockstep_supported).  DESIGN.md,
"adding a term", says what a new term needs beside its row."""
from __future__ import annotations

import dataclasses
import math
import os
from ctypes import c_float
from typing import Callable, Dict, Tuple

import numpy as np
import torch

from ._lib import check
from .body_model import CAPSULE_PAIRS_MAX, CAPSULES_MAX
from .config import stage_surface
from .tracklets import tracklets_config
from .transforms import normalize_rot


# ---------------------------------------------------------------------------------------------------------------- parsers
def _weight(config: Dict, stage: str, key: str) -> float:
    """stages.<stage>.losses.<key> as a weight: absent, null or 0 = off; negative or non-finite weights are refused."""
    v = (config["stages"][stage].get("losses") or {}).get(key, 0.0)
    v = 0.0 if v is None else float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("stages.%s.losses.%s must be 0 (off) or a positive weight (got %r)" % (stage, key, v))
    return v


def stage_robust_sigma(config: Dict, stage: str) -> float:
    """EXTENSION: stages.<stage>.robust_sigma (metres) of a config -- the Geman-McClure data term of the stage
    (uuo_problem_t.robust_sigma).  Absent or 0 = off (the reference's square); negative or non-finite values are refused, and so
    is a robust term together with the soft-assignment term `soft_chamfer`, which has no robust form."""
    st = config["stages"][stage]
    v = st.get("robust_sigma", 0.0)
    v = 0.0 if v is None else float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("stages.%s.robust_sigma must be 0 (off) or a positive number of metres (got %r)" % (stage, v))
    if v > 0.0 and float((st.get("losses") or {}).get("soft_chamfer", 0.0)) != 0.0:
        raise NotImplementedError("stages.%s: robust_sigma (Geman-McClure data term) is not built for the soft-assignment "
                                  "term soft_chamfer; use one or the other" % stage)
    return v


def stage_joint_accel(config: Dict, stage: str) -> float:
    """EXTENSION: stages.<stage>.losses.joint_accel of a config -- the weight of the joint-acceleration smoothness term of the
    chamfer or marker stage (uuo_fit_set_joint_accel), in units of m^2 per frame^2 of the sequence the stage is handed.  Absent
    or 0 = off; negative or non-finite weights are refused.  (The part stage refuses the key with its other unknown losses.)"""
    return _weight(config, stage, JOINT_ACCEL.keys[0])


def stage_latent_offsets(config: Dict) -> float:
    """EXTENSION: stages.marker.losses.latent_offsets of a config -- the weight w of the latent per-marker offsets of the marker
    stage (uuo_problem_t.w_offsets): one rest-space offset per marker column, shared by all frames and skinned with the body,
    with the prior w (1/M) sum_m (|o_m| - MARKER_DISTANCE)^2.  Absent or 0 = off; negative or non-finite weights are refused.
    (The chamfer and part stages refuse the key with their other unknown losses.)"""
    return _weight(config, "marker", LATENT_OFFSETS.keys[0])


def stage_foot_lock(config: Dict, stage: str) -> float:
    """EXTENSION: stages.<stage>.losses.foot_lock of a config -- the weight of the contact-gated foot-lock term of the chamfer
    or marker stage (uuo_fit_set_foot_lock), in units of m^2 per frame^2 of the sequence the stage is handed.  Absent or 0 =
    off; negative or non-finite weights are refused.  (The part stage refuses the key with its other unknown losses.)"""
    return _weight(config, stage, FOOT_LOCK.keys[0])


#: most sole points the floor-contact term takes (uuo_fit_set_floor)
FLOOR_MAX_POINTS = 16


def stage_floor(config: Dict, stage: str) -> Dict:
    """EXTENSION: the floor-contact term of the chamfer or marker stage (uuo_fit_set_floor) as a config states it --
    stages.<stage>.losses.floor_penetration and .floor_contact (weights on m^2; absent or 0 = off; negative or non-finite
    weights are refused), stages.<stage>.floor_height (the plane's z in metres, default 0.0) and stages.<stage>.floor_points
    (null = body_model.sole_vertices of the model, or [[left vertex ids], [right vertex ids]]: at least one per foot, 2 .. 16 in
    all; for a real SMPL the heel and toe picks extra_joint_vids[5:11] are a sensible explicit choice).  Returns
    {"w_pen", "w_con", "height", "points"}.  (The part stage refuses the keys with its other unknown losses.)"""
    st = config["stages"][stage]
    out = {"w_pen": _weight(config, stage, FLOOR.keys[0]), "w_con": _weight(config, stage, FLOOR.keys[1])}
    h = st.get("floor_height", 0.0)
    h = 0.0 if h is None else float(h)
    if not math.isfinite(h):
        raise ValueError("stages.%s.floor_height must be a finite number of metres (got %r)" % (stage, h))
    out["height"] = h
    pts = st.get("floor_points", None)
    if pts is not None:
        ok = isinstance(pts, (list, tuple)) and len(pts) == 2 and all(isinstance(r, (list, tuple)) and len(r) >= 1 for r in pts)
        ok = ok and all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for r in pts for v in r)
        if not ok or not 2 <= len(pts[0]) + len(pts[1]) <= FLOOR_MAX_POINTS:
            raise ValueError("stages.%s.floor_points must be null or [[left vertex ids], [right vertex ids]] with at least one "
                             "id >= 0 per foot and 2 .. %d in all (got %r)" % (stage, FLOOR_MAX_POINTS, pts))
        pts = [list(pts[0]), list(pts[1])]
    out["points"] = pts
    return out


def stage_capsules(config: Dict, stage: str) -> Dict:
    """EXTENSION: the bone-capsule self-penetration term of the chamfer or marker stage (uuo_fit_set_capsules) as a config
    states it -- stages.<stage>.losses.self_penetration (a weight on m^2; absent or 0 = off; negative or non-finite weights are
    refused) and stages.<stage>.capsules: null (body_model.body_capsules of the model) or {joints: [[u, v], ...] (two
    different SMPL joints < 24), geom: [[alpha, beta, radius], ...] (finite, radius > 0), pairs: [[i, j], ...] (two different
    capsule indices)} with 1 .. 32 capsules and 1 .. 256 pairs.  Returns {"w", "capsules"}.  (The part stage refuses the key
    with its other unknown losses.)"""
    v = _weight(config, stage, CAPSULES.keys[0])
    caps = config["stages"][stage].get("capsules", None)
    if caps is not None:
        def rows(x, n):
            return isinstance(x, (list, tuple)) and len(x) >= 1 and all(isinstance(r, (list, tuple)) and len(r) == n for r in x)

        def ints(x):
            return all(isinstance(q, int) and not isinstance(q, bool) for r in x for q in r)

        ok = isinstance(caps, dict) and set(caps) == {"joints", "geom", "pairs"} and rows(caps["joints"], 2) and \
            rows(caps["geom"], 3) and rows(caps["pairs"], 2) and len(caps["joints"]) == len(caps["geom"]) and \
            len(caps["joints"]) <= CAPSULES_MAX and len(caps["pairs"]) <= CAPSULE_PAIRS_MAX and ints(caps["joints"]) and \
            ints(caps["pairs"])
        if ok:
            C = len(caps["joints"])
            ok = all(0 <= u < 24 and 0 <= w < 24 and u != w for u, w in caps["joints"]) and \
                all(0 <= i < C and 0 <= j < C and i != j for i, j in caps["pairs"]) and \
                all(isinstance(q, (int, float)) and not isinstance(q, bool) and math.isfinite(q) for r in caps["geom"] for q in r) and \
                all(r[2] > 0 for r in caps["geom"])
        if not ok:
            raise ValueError("stages.%s.capsules must be null or {joints: [[u, v], ...], geom: [[alpha, beta, radius], ...], "
                             "pairs: [[i, j], ...]} with 1 .. %d capsules on two different joints < 24, finite geometry with "
                             "radius > 0, and 1 .. %d pairs of two different capsule indices (got %r)"
                             % (stage, CAPSULES_MAX, CAPSULE_PAIRS_MAX, caps))
        caps = {"joints": [list(r) for r in caps["joints"]], "geom": [[float(q) for q in r] for r in caps["geom"]],
                "pairs": [list(r) for r in caps["pairs"]]}
    return {"w": v, "capsules": caps}


def stage_joint_limits(config: Dict, stage: str) -> Dict:
    """EXTENSION: the joint-angle limit term of the chamfer or marker stage (uuo_fit_set_joint_limits) as a config states it --
    stages.<stage>.losses.joint_limits (a weight on rad^2; absent or 0 = off; negative or non-finite weights are refused) and
    stages.<stage>.joint_limits: null (body_model.smpl_joint_limits()) or {lo: [[x, y, z] x 23], hi: [[x, y, z] x 23]} in
    radians on the components of each body joint's axis-angle vector (row j - 1 is SMPL joint j; -.inf / .inf = no bound;
    lo <= hi, no NaN, lo < +inf, hi > -inf).  Returns {"w", "limits"}.  (The part stage refuses the key with its other unknown
    losses.)"""
    v = _weight(config, stage, LIMITS.keys[0])
    lim = config["stages"][stage].get("joint_limits", None)
    if lim is not None:
        def table(x):
            return isinstance(x, (list, tuple)) and len(x) == 23 and \
                all(isinstance(r, (list, tuple)) and len(r) == 3 and
                    all(isinstance(q, (int, float)) and not isinstance(q, bool) and not math.isnan(q) for q in r) for r in x)

        ok = isinstance(lim, dict) and set(lim) == {"lo", "hi"} and table(lim["lo"]) and table(lim["hi"])
        if ok:
            ok = all(a <= b and a < math.inf and b > -math.inf for ra, rb in zip(lim["lo"], lim["hi"]) for a, b in zip(ra, rb))
        if not ok:
            raise ValueError("stages.%s.joint_limits must be null or {lo: [[x, y, z] x 23], hi: [[x, y, z] x 23]} in radians with "
                             "lo <= hi, no NaN, lo < +inf and hi > -inf (-.inf / .inf = no bound; got %r)" % (stage, lim))
        lim = {"lo": [[float(q) for q in r] for r in lim["lo"]], "hi": [[float(q) for q in r] for r in lim["hi"]]}
    return {"w": v, "limits": lim}


def stage_pose_gmm(config: Dict, stage: str) -> Dict:
    """EXTENSION: the mixture pose prior of the chamfer or marker stage (uuo_fit_set_pose_gmm) as a config states it --
    stages.<stage>.losses.pose_gmm (a weight on the mixture's negative log-likelihood, in nats; absent or 0 = off; negative or
    non-finite weights are refused) and the optional stages.<stage>.pose_gmm: null or {path: null | "synthetic" | a file}:
    where the mixture comes from when the call passes none (`pose_mixture=`) -- an .npz or SMPLify-style pickle with means,
    covars, weights (body_model.load_pose_mixture), or "synthetic", the stand-in synthetic.pose_mixture().  Returns {"w",
    "path", "mixture"}; "mixture" is None until the stage's terms resolve it (StageTerms.arm_pose_mixture).  (The part stage
    refuses the key with its other unknown losses.)"""
    v = _weight(config, stage, POSE_GMM.keys[0])
    blk = config["stages"][stage].get("pose_gmm", None)
    path = None
    if blk is not None:
        what = "stages.%s.pose_gmm" % stage
        if not isinstance(blk, dict) or set(blk) - {"path"}:
            raise ValueError("%s must be null or {path} (got %r)" % (what, blk))
        path = blk.get("path", None)
        if path is not None and (not isinstance(path, str) or not path):
            raise ValueError("%s.path must be null, \"synthetic\" or a file name (got %r)" % (what, path))
    return {"w": v, "path": path, "mixture": None}


def check_pose_mixture_arg(pose_mixture):
    """EXTENSION: a call's `pose_mixture` -- None, a path (body_model.load_pose_mixture) or a dict {means [K, 69], covars
    [K, 69, 69], weights [K]} -- as body_model.prepare_pose_mixture's float32 (means, chol, offsets), or None.  ValueError
    before anything touches the device."""
    if pose_mixture is None:
        return None
    from .body_model import load_pose_mixture, prepare_pose_mixture

    if isinstance(pose_mixture, (str, bytes)) or hasattr(pose_mixture, "__fspath__"):
        pose_mixture = load_pose_mixture(pose_mixture)
    if not isinstance(pose_mixture, dict) or not {"means", "covars", "weights"} <= set(pose_mixture):
        raise ValueError("pose_mixture: a path or a dict {means, covars, weights} expected (got %s)" %
                         (sorted(pose_mixture) if isinstance(pose_mixture, dict) else type(pose_mixture).__name__))
    return prepare_pose_mixture(pose_mixture["means"], pose_mixture["covars"], pose_mixture["weights"])


def resolved_mixture(gmm: Dict, stage: str = "<stage>"):
    """stage_pose_gmm's record with its mixture in place: the call's (arm_pose_mixture), else the config's path.  A positive
    weight with neither is a ValueError."""
    if gmm["mixture"] is None and float(gmm["w"]) > 0.0:
        if gmm["path"] is None:
            raise ValueError("stages.%s.losses.pose_gmm: a positive weight needs a mixture -- pass pose_mixture= (a dict {means, "
                             "covars, weights} or a path) to multimodal_video_mocap / optim_chamfer / optim_markers, or name one in "
                             "the config (stages.%s.pose_gmm: {path: FILE | synthetic})" % (stage, stage))
        gmm["mixture"] = _mixture_of_path(gmm["path"])
    return gmm["mixture"]


#: the prepared mixtures of the config paths seen so far: every optim_chamfer / optim_markers call parses its config anew, and
#: reading and factoring a file (an inverse and a Cholesky per component) once per solve would be paid by every fit.  A file is
#: keyed by its path, size and modification time, so a rewritten file is read again.
_PATH_MIXTURES = {}


def _mixture_of_path(path: str):
    """The prepared (means, chol, offsets) of stages.<stage>.pose_gmm.path: "synthetic" or a file, read and factored once."""
    if path == "synthetic":
        key = ("synthetic",)
    else:
        try:
            st = os.stat(path)
            key = (os.path.abspath(path), st.st_size, st.st_mtime_ns)
        except OSError:
            key = None  # (load_pose_mixture names the file and the fault)
    if key is None or key not in _PATH_MIXTURES:
        if path == "synthetic":
            from .synthetic import pose_mixture

            mixture = check_pose_mixture_arg(pose_mixture())
        else:
            mixture = check_pose_mixture_arg(path)
        if key is None:
            return mixture
        _PATH_MIXTURES[key] = mixture
    return _PATH_MIXTURES[key]


def stage_pose_accel(config: Dict, stage: str) -> Dict:
    """EXTENSION: the pose-acceleration term of the chamfer or marker stage (losses.pose_accel_loss) as a config states it --
    stages.<stage>.losses.pose_accel (a weight on rad^2 per frame^4: it belongs to the frame rate; absent or 0 = off; negative or
    non-finite weights are refused) and the optional stages.<stage>.pose_accel: null or {joint_weights: null | [23 floats]},
    finite values >= 0 (entry j - 1 is SMPL joint j; null = ones).  Returns {"w", "joint_weights"}.  (The part stage refuses the
    key with its other unknown losses.)"""
    v = _weight(config, stage, POSE_ACCEL.keys[0])
    blk = config["stages"][stage].get("pose_accel", None)
    jw = None
    if blk is not None:
        what = "stages.%s.pose_accel" % stage
        if not isinstance(blk, dict) or set(blk) - {"joint_weights"}:
            raise ValueError("%s must be null or {joint_weights} (got %r)" % (what, blk))
        jw = blk.get("joint_weights", None)
        if jw is not None:
            number = lambda q: isinstance(q, (int, float)) and not isinstance(q, bool) and math.isfinite(q)
            if not isinstance(jw, (list, tuple)) or len(jw) != 23 or not all(number(q) and q >= 0.0 for q in jw):
                raise ValueError("%s.joint_weights must be null or 23 finite values >= 0 (got %r)" % (what, jw))
            jw = [float(q) for q in jw]
    return {"w": v, "joint_weights": jw}


def stage_prior_confidence(config: Dict, stage: str):
    """EXTENSION: the per-(frame, joint) confidence in the video's pose of the chamfer or marker stage as a config states it --
    stages.<stage>.prior_confidence: absent or null = off (returns None), else {gap_weight: 0.0, ramp: 0, joint_weights: null}:
    `gap_weight` in [0, 1], the weight of the pose prior in frames the video did not see; `ramp`, an integer >= 0, the number of
    unseen frames next to a seen one over which the weight falls from 1 to it; `joint_weights`, null (ones) or 23 finite values
    >= 0 (entry j - 1 is SMPL joint j).  Every key may be left out; unknown keys, and values outside these ranges, are a
    ValueError.  Returns {"gap_weight", "ramp", "joint_weights"} (prior_weight_table's `block`).  A block next to a
    reg_pose_body that is absent or 0 is allowed and changes nothing."""
    blk = config["stages"][stage].get("prior_confidence", None)
    if blk is None:
        return None
    what = "stages.%s.prior_confidence" % stage
    if not isinstance(blk, dict) or set(blk) - {"gap_weight", "ramp", "joint_weights"}:
        raise ValueError("%s must be null or {gap_weight, ramp, joint_weights} (got %r)" % (what, blk))
    number = lambda q: isinstance(q, (int, float)) and not isinstance(q, bool) and math.isfinite(q)
    gw = blk.get("gap_weight", 0.0)
    if not number(gw) or gw < 0.0 or gw > 1.0:
        raise ValueError("%s.gap_weight must be a number in [0, 1] (got %r)" % (what, gw))
    ramp = blk.get("ramp", 0)
    if not isinstance(ramp, int) or isinstance(ramp, bool) or ramp < 0:
        raise ValueError("%s.ramp must be an integer >= 0 (got %r)" % (what, ramp))
    jw = blk.get("joint_weights", None)
    if jw is not None:
        if not isinstance(jw, (list, tuple)) or len(jw) != 23 or not all(number(q) and q >= 0.0 for q in jw):
            raise ValueError("%s.joint_weights must be null or 23 finite values >= 0 (got %r)" % (what, jw))
        jw = [float(q) for q in jw]
    return {"gap_weight": float(gw), "ramp": int(ramp), "joint_weights": jw}


#: joints of the key-point reprojection term: the 24 kinematic joints
KEYPOINTS_2D_JOINTS = 24


def stage_keypoints_2d(config: Dict, stage: str) -> Dict:
    """EXTENSION: the 2D key-point reprojection term of the chamfer or marker stage (uuo_fit_set_keypoints2d) as a config states
    it -- stages.<stage>.losses.keypoints_2d (a weight on the camera's own squared units, pixels^2 or image-size-1 units^2;
    absent or 0 = off; negative or non-finite weights are refused) and the optional stages.<stage>.keypoints_2d: null or
    {sigma: 0.0, min_depth: 0.1, joint_weights: null}: `sigma` >= 0, the Geman-McClure scale of the residual in the camera's
    units (0 = the square); `min_depth` > 0, the least camera depth at which a joint counts; `joint_weights`, null (ones) or 24
    finite values >= 0 that multiply the confidences (entry j is SMPL joint j).  Every key may be left out; unknown keys, and
    values outside these ranges, are a ValueError.  Returns {"w", "sigma", "min_depth", "joint_weights"}.  The evidence itself --
    cameras, targets, confidences -- is the `keypoints_2d` record of the call (check_keypoints_2d).  (The part stage refuses
    the key with its other unknown losses.)"""
    v = _weight(config, stage, KEYPOINTS.keys[0])
    blk = config["stages"][stage].get("keypoints_2d", None)
    sigma, min_depth, jw = 0.0, 0.1, None
    if blk is not None:
        what = "stages.%s.keypoints_2d" % stage
        if not isinstance(blk, dict) or set(blk) - {"sigma", "min_depth", "joint_weights"}:
            raise ValueError("%s must be null or {sigma, min_depth, joint_weights} (got %r)" % (what, blk))
        number = lambda q: isinstance(q, (int, float)) and not isinstance(q, bool) and math.isfinite(q)
        sigma = blk.get("sigma", 0.0)
        if not number(sigma) or sigma < 0.0 or (sigma != 0.0 and not 1e-18 <= sigma <= 1e18):
            raise ValueError("%s.sigma must be 0 (the square) or a positive finite number in [1e-18, 1e18] (got %r)" % (what, sigma))
        min_depth = blk.get("min_depth", 0.1)
        if not number(min_depth) or not min_depth > 0.0:
            raise ValueError("%s.min_depth must be a positive finite number (got %r)" % (what, min_depth))
        jw = blk.get("joint_weights", None)
        if jw is not None:
            if not isinstance(jw, (list, tuple)) or len(jw) != KEYPOINTS_2D_JOINTS or not all(number(q) and q >= 0.0 for q in jw):
                raise ValueError("%s.joint_weights must be null or %d finite values >= 0 (got %r)" % (what, KEYPOINTS_2D_JOINTS, jw))
            jw = [float(q) for q in jw]
    return {"w": v, "sigma": float(sigma), "min_depth": float(min_depth), "joint_weights": jw}


def check_keypoints_2d(record, num_frames=None):
    """EXTENSION: the key-point reprojection term's evidence as float32 host tensors (None stays None): a record {"camera"
    [F, 16] (A 3x3 row-major, b, fx, fy, cx, cy: a pinhole camera per frame in world axes, p = A J + b), "targets" [F, 24, 2],
    "confidence" [F, 24]}.  The keys, the shapes, finiteness and confidence >= 0 are checked on the host: ValueError before
    anything touches the device."""
    if record is None:
        return None
    if not isinstance(record, dict) or set(record) != {"camera", "targets", "confidence"}:
        raise ValueError("keypoints_2d: a record {camera, targets, confidence} expected (got %s)" %
                         (sorted(record) if isinstance(record, dict) else type(record).__name__))
    out = {k: torch.as_tensor(v).detach().to(device="cpu", dtype=torch.float32).contiguous() for k, v in record.items()}
    F = int(out["camera"].shape[0]) if out["camera"].dim() >= 1 else -1
    want = {"camera": (F, 16), "targets": (F, KEYPOINTS_2D_JOINTS, 2), "confidence": (F, KEYPOINTS_2D_JOINTS)}
    if F < 1 or (num_frames is not None and F != int(num_frames)) or any(tuple(out[k].shape) != want[k] for k in want):
        raise ValueError("keypoints_2d: camera [F, 16], targets [F, 24, 2] and confidence [F, 24] with the markers' F = %s "
                         "expected (got %s)" % (num_frames, {k: tuple(out[k].shape) for k in sorted(out)}))
    if not all(bool(torch.isfinite(out[k]).all()) for k in out):
        raise ValueError("keypoints_2d: finite cameras, targets and confidences expected")
    if bool((out["confidence"] < 0.0).any()):
        raise ValueError("keypoints_2d: confidences >= 0 expected")
    return out


def armed_keypoints(record, kp: Dict):
    """check_keypoints_2d's record as the solvers use it, with stage_keypoints_2d's record `kp`: the confidences times the joint
    weights -- or None when there is no record, the weight is 0 or no confidence * joint weight is positive: nothing is armed,
    every route and every kernel is the plain one (the foot-lock term's rule for a capture without contacts)."""
    if record is None or float(kp["w"]) == 0.0:
        return None
    conf = record["confidence"]
    if kp["joint_weights"] is not None:
        conf = (conf * torch.tensor(kp["joint_weights"], dtype=torch.float32)[None, :]).contiguous()
    if not bool((conf > 0.0).any()):
        return None
    return {"camera": record["camera"], "targets": record["targets"], "confidence": conf}


def prior_weight_table(seen, block: Dict) -> torch.Tensor:
    """EXTENSION: the pose prior's weights [F, 23] float32 (host) from `seen` [F] (mocap frames the video saw; anything
    non-zero counts) and stage_prior_confidence's record:  omega[t, j] = frame_w[t] * joint_weights[j],  d[t] the distance in
    frames to the nearest seen frame,  frame_w[t] = 1 where d = 0, else max(gap_weight, 1 - d / (ramp + 1)).  ramp = 0 makes
    every unseen frame gap_weight; ramp = 2 tapers 2/3, 1/3.  No seen frame at all is a ValueError."""
    sn = torch.as_tensor(seen).detach().cpu().reshape(-1) != 0
    F = int(sn.shape[0])
    idx = torch.nonzero(sn).reshape(-1).to(torch.int64)
    if idx.numel() == 0:
        raise ValueError("prior_weight_table: the video saw no frame at all")
    t = torch.arange(F, dtype=torch.int64)
    d = (t[:, None] - idx[None, :]).abs().min(dim=1)[0].to(torch.float64)
    gw, ramp = float(block["gap_weight"]), int(block["ramp"])
    fw = torch.where(d == 0, torch.ones_like(d), torch.clamp(1.0 - d / (ramp + 1.0), min=gw))
    jw = block.get("joint_weights")
    jw = torch.ones(23, dtype=torch.float64) if jw is None else torch.tensor([float(q) for q in jw], dtype=torch.float64)
    return (fw[:, None] * jw[None, :]).to(torch.float32).contiguous()


def check_prior_weights(prior_weights, num_frames=None):
    """EXTENSION: the pose prior's weights as a float32 host tensor [F, 23] (None stays None).  Shape, finiteness and >= 0 are
    checked on the host: ValueError before anything touches the device."""
    if prior_weights is None:
        return None
    w = torch.as_tensor(prior_weights).detach().to(device="cpu", dtype=torch.float32)
    if w.dim() != 2 or w.shape[1] != 23 or (num_frames is not None and w.shape[0] != int(num_frames)):
        raise ValueError("prior_weights: [F, 23] with the markers' F = %s expected (got %s)" % (num_frames, tuple(w.shape)))
    if not bool(torch.isfinite(w).all()) or bool((w < 0.0).any()):
        raise ValueError("prior_weights: finite weights >= 0 expected")
    return w


def check_foot_contacts(foot_contacts, num_frames=None):
    """EXTENSION: the foot-lock term's contact labels as a float32 host tensor [F, 2] (left, right foot; None stays None).
    Shape, finiteness and the range [0, 1] are checked on the host: ValueError before anything touches the device."""
    if foot_contacts is None:
        return None
    c = torch.as_tensor(foot_contacts).detach().to(device="cpu", dtype=torch.float32)
    if c.dim() != 2 or c.shape[1] != 2 or (num_frames is not None and c.shape[0] != int(num_frames)):
        raise ValueError("foot_contacts: [F, 2] with the markers' F = %s expected (got %s)" % (num_frames, tuple(c.shape)))
    if not bool(torch.isfinite(c).all()) or bool((c < 0.0).any()) or bool((c > 1.0).any()):
        raise ValueError("foot_contacts: finite labels in [0, 1] expected")
    return c


def armed_weights(weights):
    """check_prior_weights' table as the solvers use it: None, or a table of ones, is None everywhere -- nothing is armed, every
    route and every kernel is the plain one."""
    return None if weights is None or bool((weights == 1.0).all()) else weights


# ------------------------------------------------------------------------- default tables and what the labels leave of a term
def floor_points(floor: Dict, tables):
    """stage_floor's sole points as (vertex ids, the left foot's first; number of left points; number of right points):
    the configured ones, or body_model.sole_vertices of the model."""
    pts = floor["points"]
    if pts is None:
        from .body_model import sole_vertices

        pts = sole_vertices(tables)
    return [int(v) for v in pts[0]] + [int(v) for v in pts[1]], len(pts[0]), len(pts[1])


def floor_weights(floor: Dict, contacts):
    """(floor_penetration, floor_contact) as they act: floor_contact counts only with labels that hold a contact."""
    w_pen, w_con = float(floor["w_pen"]), float(floor["w_con"])
    if contacts is None or not bool(contacts.any()):
        w_con = 0.0
    return w_pen, w_con


def capsule_lists(caps: Dict, tables):
    """stage_capsules' (joints, geometry, pairs): the configured lists, or body_model.body_capsules of the model."""
    lists = caps["capsules"]
    if lists is None:
        from .body_model import body_capsules

        return body_capsules(tables)
    return lists["joints"], lists["geom"], lists["pairs"]


def limit_tables(lim: Dict):
    """stage_joint_limits' (lo, hi): the configured tables, or body_model.smpl_joint_limits()."""
    if lim["limits"] is None:
        from .body_model import smpl_joint_limits

        return smpl_joint_limits()
    return lim["limits"]["lo"], lim["limits"]["hi"]


# ------------------------------------------------------------------------------- a term's state on a stage problem (`set`)
def _set_joint_accel(p, w, contacts, weights, keypoints, smpl_inference):
    p.joint_accel = w


def _set_foot_lock(p, w, contacts, weights, keypoints, smpl_inference):
    """Keeps a contiguous float32 device copy of the checked contact labels and the weight the workspace is armed with: `w` when
    the labels gate at least one (frame pair, foot), else 0 -- a capture without video contacts (no labels, or none that holds
    over two consecutive frames) runs the plain kernels, bit for bit."""
    if contacts is None:
        return
    p.foot_contacts = contacts.to(device=p.device, dtype=torch.float32).contiguous()
    if w > 0.0 and p.F >= 2 and bool((contacts[1:] * contacts[:-1]).any()):
        p.foot_lock = float(w)


def _set_floor(p, floor, contacts, weights, keypoints, smpl_inference):
    """Keeps the sole points' vertex ids and the contact labels on the device, and the weights the workspace is armed with
    (floor_weights).  With both 0 nothing is armed -- the model's tables are not even looked at -- and the problem runs the plain
    kernels, bit for bit."""
    w_pen, w_con = floor_weights(floor, contacts)
    if w_pen == 0.0 and w_con == 0.0:
        return
    vids, p.floor_kl, p.floor_kr = floor_points(floor, smpl_inference.tables)
    if max(vids) >= p.model.V:
        raise ValueError("floor_points: a vertex id is past the model's %d vertices" % p.model.V)
    p.floor_vids = torch.tensor(vids, dtype=torch.int32, device=p.device)
    p.floor_pen, p.floor_con, p.floor_height = w_pen, w_con, float(floor["height"])
    if w_con != 0.0:
        p.floor_contacts = contacts.to(device=p.device, dtype=torch.float32).contiguous()


def _set_capsules(p, caps, contacts, weights, keypoints, smpl_inference):
    """Keeps the weight and contiguous HOST copies of the capsule lists, which the library checks and copies at the call.  With
    weight 0 nothing is armed and the problem runs the plain kernels, bit for bit."""
    if float(caps["w"]) == 0.0:
        return
    lists = capsule_lists(caps, smpl_inference.tables)
    p.cap_joints = np.ascontiguousarray(np.asarray(lists[0], dtype=np.int32).reshape(-1, 2))
    p.cap_geom = np.ascontiguousarray(np.asarray(lists[1], dtype=np.float32).reshape(-1, 3))
    p.cap_pairs = np.ascontiguousarray(np.asarray(lists[2], dtype=np.int32).reshape(-1, 2))
    p.cap_w = float(caps["w"])


def _set_joint_limits(p, lim, contacts, weights, keypoints, smpl_inference):
    """Keeps the weight and contiguous HOST copies of the two tables (row j - 1 is SMPL joint j; -inf / +inf = no bound), which
    the library checks and copies at the call.  With weight 0 nothing is armed."""
    if float(lim["w"]) == 0.0:
        return
    lo, hi = limit_tables(lim)
    p.lim_lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float32).reshape(23, 3))
    p.lim_hi = np.ascontiguousarray(np.asarray(hi, dtype=np.float32).reshape(23, 3))
    p.lim_w = float(lim["w"])


def _set_pose_gmm(p, gmm, contacts, weights, keypoints, smpl_inference):
    """Keeps the weight and the three HOST arrays of the prepared mixture (float32: means [K, 69], factors [K, 69, 69],
    offsets [K]), which the library checks and copies at the call.  With weight 0 nothing is armed."""
    if float(gmm["w"]) == 0.0:
        return
    p.gmm_means, p.gmm_chol, p.gmm_offsets = resolved_mixture(gmm, "chamfer" if p.stage == 0 else "marker")
    p.gmm_w = float(gmm["w"])


def _set_prior_weights(p, block, contacts, weights, keypoints, smpl_inference):
    """`weights` is check_prior_weights' host tensor (or None); what armed_weights leaves of it goes to the device, where the
    library reads it at every evaluation."""
    if armed_weights(weights) is not None:
        p.prior_weights = weights.to(device=p.device, dtype=torch.float32).contiguous()


def _set_keypoints(p, kp, contacts, weights, keypoints, smpl_inference):
    """`keypoints` is armed_keypoints' record of the call (or None: nothing is armed).  Its three tables go to the device, where
    the library reads them at every evaluation."""
    if keypoints is None:
        return
    dev = lambda t: t.to(device=p.device, dtype=torch.float32).contiguous()
    p.kp_cam, p.kp_targets, p.kp_conf = dev(keypoints["camera"]), dev(keypoints["targets"]), dev(keypoints["confidence"])
    p.kp_w, p.kp_sigma, p.kp_min_depth = float(kp["w"]), float(kp["sigma"]), float(kp["min_depth"])


def _set_pose_accel(p, pacc, contacts, weights, keypoints, smpl_inference):
    """Keeps the weight and a contiguous HOST copy of the joint weights (None = ones), which the library checks and copies at the
    call.  With weight 0 nothing is armed.  (A problem is built with a non-zero weight only under execution.pose_accel_fused:
    StageTerms.check_problem.)"""
    if float(pacc["w"]) == 0.0:
        return
    if pacc["joint_weights"] is not None:
        p.pacc_u = np.ascontiguousarray(np.asarray(pacc["joint_weights"], dtype=np.float32).reshape(23))
    p.pacc_w = float(pacc["w"])


# ---------------------------------------------------------------- a term on the closures composed from the operators (`composed`)
def _composed_joint_accel(w, losses, contacts, smpl_inference, keypoints=None):
    from .losses import joint_accel_loss

    if JOINT_ACCEL.keys[0] not in losses:  # (the key's presence, not a positive weight)
        return None
    return "joints", lambda joints: joint_accel_loss(joints) * w


def _composed_foot_lock(w, losses, contacts, smpl_inference, keypoints=None):
    from .losses import foot_lock_loss

    if not w > 0.0 or contacts is None:  # (whenever labels were passed, whether or not they gate a frame pair)
        return None
    return "joints", lambda joints: foot_lock_loss(joints, contacts) * w


def _composed_floor(floor, losses, contacts, smpl_inference, keypoints=None):
    from .losses import floor_loss

    w_pen, w_con = floor_weights(floor, contacts)
    if w_pen == 0.0 and w_con == 0.0:
        return None
    vids, k_left, _ = floor_points(floor, smpl_inference.tables)
    return "vertices", lambda vertices: floor_loss(vertices, vids, k_left, contacts, floor["height"], w_pen, w_con)


def _composed_capsules(caps, losses, contacts, smpl_inference, keypoints=None):
    from .losses import self_penetration_loss

    if caps["w"] == 0.0:
        return None
    cj, cg, pr = capsule_lists(caps, smpl_inference.tables)
    return "joints", lambda joints: self_penetration_loss(joints, cj, cg, pr, caps["w"])


def _composed_limits(lim, losses, contacts, smpl_inference, keypoints=None):
    from .losses import joint_limit_loss

    if lim["w"] == 0.0:
        return None
    lo, hi = limit_tables(lim)
    return "rot_body", lambda rot_body: joint_limit_loss(rot_body, lo, hi, lim["w"])


def _composed_pose_gmm(gmm, losses, contacts, smpl_inference, keypoints=None):
    from .losses import pose_gmm_loss

    if gmm["w"] == 0.0:
        return None
    means, chol, offsets = resolved_mixture(gmm)
    return "rot_body", lambda rot_body: pose_gmm_loss(rot_body, means, chol, offsets, gmm["w"])


def _composed_pose_accel(pacc, losses, contacts, smpl_inference, keypoints=None):
    from .losses import pose_accel_loss

    if pacc["w"] == 0.0:
        return None
    return "rot_body", lambda rot_body: pose_accel_loss(rot_body, pacc["w"], pacc["joint_weights"])


def _composed_keypoints(kp, losses, contacts, smpl_inference, keypoints=None):
    from .losses import keypoints_2d_loss

    if keypoints is None:  # (armed_keypoints: no record, weight 0 or no positive confidence)
        return None
    cache = {}

    def term(joints):
        key = (joints.device, joints.dtype)
        if key not in cache:
            cache[key] = [keypoints[k].to(device=joints.device, dtype=joints.dtype) for k in ("camera", "targets", "confidence")]
        return keypoints_2d_loss(joints, *cache[key], kp["w"], kp["sigma"], kp["min_depth"])

    return "joints", term


# ------------------------------------------------------------------------------------------------------------- the table
_SHARDING = "frame-block sharding (parallel.shard_frames)"
_COUPLES = "stages.%%s.losses.%s (extension) couples neighbouring frames, across the ranks' frame blocks too: it is not built for " + _SHARDING
_SOFT = "stages.chamfer: the fused %s is not built for the soft-assignment closure; optim_chamfer composes that combination from " \
        "the operators"


@dataclasses.dataclass(eq=False)
class Term:
    """One row of TERMS: everything the host layer knows about one extension term."""
    name: str                  # what the refusals call the term
    parse: Callable            # (config, stage) -> the term's record as the config states it
    on: Callable               # record -> True when the config turns the term on
    keys: Tuple[str, ...] = ()  # its loss keys (none: the term is a key of the stage itself)
    label: str = None          # how the refusals spell the keys
    stages: Tuple[str, ...] = ("chamfer", "marker")
    switch: str = None         # the `execution.*` key that, set False, sends the term to the composed closure (None: one route only)
    opt_in: bool = False       # True: the switch is False when absent -- the term runs composed unless the config asks for the fused closure
    batch: bool = False        # True: a lock-step batch carries the term (on its fused closure)
    # the term on a stage problem: the attribute (dotted path) that is non-zero when the problem carries it, the attributes it
    # keeps with their off values, set(problem, record, contacts, weights, keypoints, smpl_inference) at construction -- the
    # checked contact labels, prior weights and armed key-point record of the call -- and the library call
    # that arms a workspace, with its arguments off and on(problem)
    flag: str = None
    state: Dict = dataclasses.field(default_factory=dict)
    set: Callable = None
    setter: str = None
    off_args: tuple = ()
    on_args: Callable = None
    # refusal texts: under frame-block sharding (%s = the stage), raised by the sharded solve itself or -- sharded_by_route -- on the
    # way to it; of the fused soft-assignment closure; of the per-frame vertex table; of a stage problem without a closure for it
    sharded: str = None
    sharded_by_route: bool = False
    soft: str = None
    frame_table: str = None
    no_closure: str = None
    fused_only: str = None     # ... or of every route but the plain fused closures, whichever it is (%s = the route)
    # (record, losses, contacts, smpl_inference, keypoints=None) -> None | (input, function): the term on the composed closures, a
    # function of "joints" (joints[:, :24]), "vertices" or "rot_body" (normalize_rot(p_pose))
    composed: Callable = None

    def __post_init__(self):
        self.label = self.label or " / ".join(self.keys)

    def carried_by(self, problem) -> bool:
        """True when `problem` (a stage problem, or a stand-in that has only some of the attributes) carries the term."""
        v = problem
        for attr in self.flag.split("."):
            v = getattr(v, attr, 0.0)
        return bool(v)

    def arm(self, problem):
        """The term's one library call on the problem's workspace: off, or on with the problem's state."""
        args = self.on_args(problem) if self.carried_by(problem) else self.off_args
        check(getattr(problem.lib, self.setter)(problem.fit, *args), self.setter)


def batch_refusal_text(name: str, label: str) -> str:
    return "lock-step batches do not carry %s (%s, extension): solve such problems one by one" % (name, label)


ROBUST = Term("the Geman-McClure data term", stage_robust_sigma, lambda v: v > 0.0, label="robust_sigma",
              switch="robust_fused", batch=True)
JOINT_ACCEL = Term(
    "the joint-acceleration term", stage_joint_accel, lambda v: v > 0.0, keys=("joint_accel",), switch="temporal_fused",
    flag="joint_accel", state={"joint_accel": 0.0}, set=_set_joint_accel,
    setter="uuo_fit_set_joint_accel", off_args=(c_float(0.0),), on_args=lambda p: (c_float(p.joint_accel),),
    sharded=_COUPLES % "joint_accel", soft=_SOFT % "joint-acceleration term (joint_accel)", composed=_composed_joint_accel)
LATENT_OFFSETS = Term(
    "the latent marker offsets", lambda config, stage: stage_latent_offsets(config), lambda v: v > 0.0, keys=("latent_offsets",),
    stages=("marker",), flag="problem.w_offsets",
    fused_only="stages.marker.losses.latent_offsets (latent marker offsets, extension) is built for the fused marker closures only, "
            "not for %s")
FOOT_LOCK = Term(
    "the foot-lock term", stage_foot_lock, lambda v: v > 0.0, keys=("foot_lock",), switch="temporal_fused",
    flag="foot_lock", state={"foot_lock": 0.0, "foot_contacts": None}, set=_set_foot_lock,
    setter="uuo_fit_set_foot_lock", off_args=(c_float(0.0), None),
    on_args=lambda p: (c_float(p.foot_lock), p.foot_contacts.data_ptr()),
    sharded=_COUPLES % "foot_lock", soft=_SOFT % "foot-lock term (foot_lock)", composed=_composed_foot_lock)
FLOOR = Term(
    "the floor-contact term", stage_floor, lambda r: r["w_pen"] > 0.0 or r["w_con"] > 0.0,
    keys=("floor_penetration", "floor_contact"), switch="floor_fused", flag="floor_on",
    # floor_vids: [K] int32 on the device, the left foot's floor_kl points first
    state={"floor_pen": 0.0, "floor_con": 0.0, "floor_height": 0.0, "floor_vids": None, "floor_kl": 0, "floor_kr": 0,
           "floor_contacts": None},
    set=_set_floor, setter="uuo_fit_set_floor", off_args=(c_float(0.0), c_float(0.0), c_float(0.0), None, 0, 0, None),
    on_args=lambda p: (c_float(p.floor_pen), c_float(p.floor_con), c_float(p.floor_height), p.floor_vids.data_ptr(), p.floor_kl,
                       p.floor_kr, p.floor_contacts.data_ptr() if p.floor_con != 0.0 else None),
    sharded="stages.%s.losses.floor_penetration / floor_contact (extension): the floor-contact term is not built for " + _SHARDING,
    soft=_SOFT % "floor-contact term (floor_penetration / floor_contact)",
    frame_table="the per-frame vertex table (tracklets, extension) is not built for the floor-contact term "
                "(stages.marker.losses.floor_penetration / floor_contact)",
    composed=_composed_floor)
CAPSULES = Term(
    "the self-penetration term", stage_capsules, lambda r: r["w"] > 0.0, keys=("self_penetration",), switch="capsule_fused",
    flag="capsules_on",
    # the three HOST lists: [C, 2] int32, [C, 3] float32 (alpha, beta, radius), [P, 2] int32 numpy
    state={"cap_w": 0.0, "cap_joints": None, "cap_geom": None, "cap_pairs": None},
    set=_set_capsules, setter="uuo_fit_set_capsules", off_args=(c_float(0.0), 0, None, None, 0, None),
    on_args=lambda p: (c_float(p.cap_w), int(p.cap_joints.shape[0]), p.cap_joints.ctypes.data, p.cap_geom.ctypes.data,
                       int(p.cap_pairs.shape[0]), p.cap_pairs.ctypes.data),
    sharded="stages.%s.losses.self_penetration (extension): the self-penetration term is not built for " + _SHARDING,
    soft=_SOFT % "self-penetration term (self_penetration)", composed=_composed_capsules)
LIMITS = Term(
    "the joint-angle limit term", stage_joint_limits, lambda r: r["w"] > 0.0, keys=("joint_limits",), switch="limit_fused",
    flag="joint_limits_on", state={"lim_w": 0.0, "lim_lo": None, "lim_hi": None},  # the two HOST tables: [23, 3] float32 numpy
    set=_set_joint_limits, setter="uuo_fit_set_joint_limits", off_args=(c_float(0.0), None, None),
    on_args=lambda p: (c_float(p.lim_w), p.lim_lo.ctypes.data, p.lim_hi.ctypes.data),
    sharded="stages.%s.losses.joint_limits (extension): the joint-angle limit term is not built for " + _SHARDING,
    soft=_SOFT % "joint-angle limit term (joint_limits)", composed=_composed_limits)
POSE_GMM = Term(
    "the pose mixture term", stage_pose_gmm, lambda r: r["w"] > 0.0, keys=("pose_gmm",), switch="pose_gmm_fused",
    flag="pose_gmm_on",
    # the three HOST arrays of the prepared mixture: [K, 69], [K, 69, 69], [K] float32 numpy
    state={"gmm_w": 0.0, "gmm_means": None, "gmm_chol": None, "gmm_offsets": None},
    set=_set_pose_gmm, setter="uuo_fit_set_pose_gmm", off_args=(c_float(0.0), 0, None, None, None),
    on_args=lambda p: (c_float(p.gmm_w), int(p.gmm_means.shape[0]), p.gmm_means.ctypes.data, p.gmm_chol.ctypes.data,
                       p.gmm_offsets.ctypes.data),
    sharded="stages.%s.losses.pose_gmm (extension): the pose mixture term is not built for " + _SHARDING,
    soft=_SOFT % "pose mixture term (pose_gmm)", composed=_composed_pose_gmm)
PRIOR = Term(
    "the pose prior's weights", stage_prior_confidence, lambda blk: blk is not None, label="prior_confidence",
    switch="prior_conf_fused", flag="prior_conf_on", state={"prior_weights": None},  # [F, 23] float32 on the device
    set=_set_prior_weights, setter="uuo_fit_set_prior_weights", off_args=(None,), on_args=lambda p: (p.prior_weights.data_ptr(),),
    sharded="stages.%s.prior_confidence (extension): the pose prior's weights are not built for " + _SHARDING,
    sharded_by_route=True,
    soft="stages.chamfer: the pose prior's weights (prior_confidence) are not built for the soft-assignment closure")
KEYPOINTS = Term(
    "the key-point reprojection term", stage_keypoints_2d, lambda r: r["w"] > 0.0, keys=("keypoints_2d",), switch="keypoints_fused",
    flag="keypoints_on",
    # the three tables on the device: cameras [F, 16], targets [F, 24, 2], confidences times joint weights [F, 24], float32
    state={"kp_w": 0.0, "kp_sigma": 0.0, "kp_min_depth": 0.0, "kp_cam": None, "kp_targets": None, "kp_conf": None},
    set=_set_keypoints, setter="uuo_fit_set_keypoints2d", off_args=(c_float(0.0), c_float(0.0), c_float(0.0), None, None, None),
    on_args=lambda p: (c_float(p.kp_w), c_float(p.kp_sigma), c_float(p.kp_min_depth), p.kp_cam.data_ptr(), p.kp_targets.data_ptr(),
                       p.kp_conf.data_ptr()),
    sharded="stages.%s.losses.keypoints_2d (extension): the key-point reprojection term is not built for " + _SHARDING,
    soft=_SOFT % "key-point reprojection term (keypoints_2d)", composed=_composed_keypoints)
POSE_ACCEL = Term(
    "the pose-acceleration term", stage_pose_accel, lambda r: r["w"] > 0.0, keys=("pose_accel",), switch="pose_accel_fused",
    opt_in=True, flag="pose_accel_on", state={"pacc_w": 0.0, "pacc_u": None},  # the HOST table: [23] float32 numpy, None = ones
    set=_set_pose_accel, setter="uuo_fit_set_pose_accel", off_args=(c_float(0.0), None),
    on_args=lambda p: (c_float(p.pacc_w), p.pacc_u.ctypes.data if p.pacc_u is not None else None),
    sharded=_COUPLES % "pose_accel", sharded_by_route=True, soft=_SOFT % "pose-acceleration term (pose_accel)",
    no_closure="stages.%s.losses.pose_accel (extension) has no fused closure without execution.pose_accel_fused: True; %s "
               "composes it from the operators",
    composed=_composed_pose_accel)

#: one row per extension term.  The order is that of the library calls in _StageProblem._arm, of the refusals of
#: engine.solve_batch and of the sharded solves, and of the terms in the composed closures' sum
TERMS = (ROBUST, JOINT_ACCEL, LATENT_OFFSETS, FOOT_LOCK, FLOOR, CAPSULES, LIMITS, POSE_GMM, PRIOR, KEYPOINTS, POSE_ACCEL)
#: the order in which a stage problem's constructor looks at the terms that can refuse it (that of its refusals, kept)
PROBLEM_ORDER = (CAPSULES, LIMITS, POSE_ACCEL, JOINT_ACCEL, FOOT_LOCK, FLOOR, POSE_GMM)

#: the reference's own loss keys of the fused closures, the data terms the chamfer stage has beside them (extensions with a
#: switch of their own: execution.chamfer_soft_fused / surface_fused), and the reference's optional chamfer-stage terms
REFERENCE_KEYS = {"chamfer": ("full_chamfer", "reg_pose_body", "reg_betas"), "marker": ("marker", "reg_pose_body", "reg_betas")}
SOFT_KEY, SURFACE_KEY = "soft_chamfer", "surface_chamfer"
REFERENCE_OPTIONAL_KEYS = ("part_chamfer", "trans_vel", "ground")


def stage_keys(stage: str) -> set:
    """The loss keys a stage's fused closures know: the reference's and the terms' (a term without a fused closure at weight 0)."""
    return set(REFERENCE_KEYS[stage]).union(*(t.keys for t in TERMS if stage in t.stages))


def problem_keys(stage: str) -> set:
    """The loss keys ChamferProblem / MarkerProblem accept (a term without a fused closure only at weight 0)."""
    return stage_keys(stage) | ({SOFT_KEY, SURFACE_KEY} if stage == "chamfer" else set())


def composed_keys(stage: str) -> set:
    """The loss keys the closures composed from the operators accept."""
    return problem_keys(stage) | (set(REFERENCE_OPTIONAL_KEYS) if stage == "chamfer" else set())


# ----------------------------------------------------------------------------------------------- a stage's terms, parsed once
class StageTerms:
    """The terms of one stage of a config: terms[ROW] is the row's parsed record, parsed at the first look and kept (so a
    refusal or a ValueError of a parser surfaces where the record is first needed, as it always has).  `prior_weights` is the
    armed table of the call (armed_weights), None when there is none; `keypoints` the armed key-point record of the call
    (arm_keypoints), None when there is none."""

    def __init__(self, config: Dict, stage: str, prior_weights=None):
        self.config, self.stage, self.prior_weights, self._records = config, stage, prior_weights, {}
        self.keypoints = None

    def arm_keypoints(self, record, num_frames=None):
        """The call's `keypoints_2d` record, checked on the host (check_keypoints_2d) and reduced to what acts
        (armed_keypoints) with the stage's block, which is parsed here whether or not there is a record.  None leaves what an
        earlier call armed.  Returns self.keypoints."""
        kp = self[KEYPOINTS]
        if record is not None:
            self.keypoints = armed_keypoints(check_keypoints_2d(record, num_frames), kp)
        return self.keypoints

    def arm_pose_mixture(self, pose_mixture=None):
        """The call's `pose_mixture` (a dict {means, covars, weights} or a path; None: the config's stages.<stage>.pose_gmm.path,
        or what an earlier call armed), checked and prepared on the host.  With the key on, a mixture must come from one of the
        two: ValueError otherwise.  Returns the prepared (means, chol, offsets) or None."""
        gmm = self[POSE_GMM]
        if pose_mixture is not None:
            gmm["mixture"] = check_pose_mixture_arg(pose_mixture)
        return resolved_mixture(gmm, self.stage) if self.on(POSE_GMM) else None

    def __getitem__(self, term: Term):
        if term not in self._records:
            self._records[term] = term.parse(self.config, self.stage)
        return self._records[term]

    def on(self, term: Term) -> bool:
        """True when the config turns the term on (a non-zero weight; for PRIOR, the block)."""
        return term.on(self[term])

    def active(self, term: Term) -> bool:
        """True when the term acts in this call: on -- PRIOR: when a table is armed, whatever the config says; KEYPOINTS: when a
        record is armed (which takes the key on)."""
        if term is KEYPOINTS:
            return self.keypoints is not None
        return self.prior_weights is not None if term is PRIOR else self.on(term)

    def execution(self, switch: str, default: bool = True) -> bool:
        return bool((self.config.get("execution") or {}).get(switch, default))

    def fused(self, term: Term) -> bool:
        """False when the term is to run on the closure composed from the operators: its switch is False (the fused closures'
        checker), or absent for a term that is opt-in.  True when it is not active: nothing to compose without the term."""
        return term.switch is None or not self.active(term) or self.execution(term.switch, not term.opt_in)

    def composed_tail(self, losses: Dict, contacts, smpl_inference):
        """The terms that the composed closures add after the reference's, as (input, function) pairs in TERMS' order."""
        pairs = [t.composed(self[t], losses, contacts, smpl_inference, keypoints=self.keypoints)
                 for t in TERMS if t.composed is not None]
        return [p for p in pairs if p is not None]

    def refuse_latent_offsets(self, route: str):
        if self.on(LATENT_OFFSETS):
            raise NotImplementedError(LATENT_OFFSETS.fused_only % route)

    def refuse_sharded(self, only=None):
        """Frame-block sharding: the refusals of the sharded solve itself (the latent offsets' last), or -- `only` -- those of
        the terms the route refuses on the way (PRIOR on the config block alone too, even without a table)."""
        for t in only or [t for t in TERMS if t.sharded and not t.sharded_by_route]:
            # (KEYPOINTS: only with an armed record -- without one the key changes nothing, a refusal included)
            if self.stage in t.stages and (self.active(t) or (self.on(t) and t is not KEYPOINTS)):
                raise NotImplementedError(t.sharded % self.stage)
        if only is None and self.stage == "marker":
            self.refuse_latent_offsets(_SHARDING)

    def check_problem(self, soft: bool):
        """A stage problem's constructor: every term parsed (its ValueError before the device is touched), and refused where
        the fused closure -- with `soft`, the soft-assignment one -- cannot carry it."""
        for t in PROBLEM_ORDER:
            if self.on(t) and t.no_closure and not self.fused(t):  # (opt-in: the problem has the closure only when asked for)
                raise NotImplementedError(t.no_closure % (self.stage, {"chamfer": "optim_chamfer", "marker": "optim_markers"}[self.stage]))
            if self.on(t) and soft:
                raise NotImplementedError(t.soft)


#: what a composed term is a function of, from the model's output and the body pose of an evaluation
_INPUTS = {"joints": lambda out, p_pose: out["joints"][:, :24], "vertices": lambda out, p_pose: out["vertices"],
           "rot_body": lambda out, p_pose: normalize_rot(p_pose)}


def add_tail(loss, tail, out: Dict, p_pose):
    """`loss` plus every term of StageTerms.composed_tail at this evaluation.  Each term takes its input afresh (its own slice,
    its own normalisation): the float sum and the autograd graph stay what they were, term by term."""
    for kind, fn in tail:
        loss = loss + fn(_INPUTS[kind](out, p_pose))
    return loss


# -------------------------------------------------------------------------------------------------------- the route decision
_FRAME_TABLE = "the per-frame vertex table (tracklets, extension)"


def stage_route(terms: StageTerms, on_device: bool, sharded: bool, shared_betas: bool = False, placement: str = None) -> str:
    """Which closure a chamfer or marker stage call runs on: "fused" (ChamferProblem / MarkerProblem), "sharded" (the fused
    solve over frame blocks) or "composed" (the closure composed from the operators) -- or the refusal of a combination that is
    not built.  Touches no device.  `terms`: the stage's terms with the call's armed prior weights;  on_device: whether the
    markers (chamfer) / the placement (marker) live on the GPU;  sharded: an active parallel.shard_frames;  shared_betas: a
    parallel.shared_betas reducer;  placement (marker): "one_hot", "three" (up to three non-zeros per row), "more" or
    "frame_table".  DESIGN.md lists what this keeps exactly as the ladders it replaces had it."""
    config, stage = terms.config, terms.stage
    st = config["stages"][stage]
    composed = lambda: any(not terms.fused(t) for t in TERMS if stage in t.stages)
    if stage == "chamfer":
        soft = float(st["losses"].get(SOFT_KEY, 0.0)) != 0.0 and on_device and terms.execution("chamfer_soft_fused")
        # (an opt-in term counts here only on its fused closure: without its switch it is not even parsed at this point, as before)
        if soft and any(terms.active(t) for t in TERMS if t.soft and (not t.opt_in or terms.execution(t.switch, False))):
            soft = False  # no instantiation of the dense backward (k_bwd_dense) carries these: composed closure, no refusal
        w_surface, _ = stage_surface(config)
        if w_surface > 0.0 and sharded:
            raise NotImplementedError("stages.chamfer.losses.surface_chamfer (point-to-surface term, extension) is not built for "
                                      + _SHARDING)
        allowed = stage_keys(stage) | ({SOFT_KEY} if soft else set())
        if w_surface == 0.0 or (on_device and terms.execution("surface_fused")):  # (weight 0 is the key absent)
            allowed.add(SURFACE_KEY)
        if (set(st["losses"]) - allowed) or not st["yaw_lock"] or composed():
            if sharded:
                terms.refuse_sharded((POSE_ACCEL,))
            return "composed"
        if sharded:
            if soft:
                raise NotImplementedError("stages.chamfer.losses.soft_chamfer (extension) is not built for " + _SHARDING +
                                          "; set execution.chamfer_soft_fused: False or use another mode")
            terms.refuse_sharded((PRIOR, POSE_ACCEL))
            return "sharded"
        return "fused"
    if placement == "frame_table":  # fused one-hot closure only
        if terms.on(FLOOR):
            raise NotImplementedError(FLOOR.frame_table)
        if composed():
            raise NotImplementedError("%s is built for the fused marker closure only, not for the closure composed from the operators "
                                      "(execution.robust_fused / temporal_fused / capsule_fused / limit_fused / prior_conf_fused: "
                                      "False; stages.marker.losses.pose_accel)" % _FRAME_TABLE)
        terms.refuse_latent_offsets(_FRAME_TABLE + ": an offset per column has no meaning once the column changes identity")
        if sharded:
            raise NotImplementedError("%s is not built for %s" % (_FRAME_TABLE, _SHARDING))
        if shared_betas:
            raise NotImplementedError("%s is not built for shared betas (parallel.shared_betas)" % _FRAME_TABLE)
        return "fused"
    if composed():
        if sharded:
            terms.refuse_sharded((POSE_ACCEL,))
        return "composed"
    # a barycentric placement has a fused closure (k_bary_fwd + k_bwd_items) when it is up to three weighted vertices per marker
    # and nothing else; execution.marker_bary_fused: False, more non-zeros in a row, or frame-block sharding keep it composed
    if placement != "one_hot" and not (on_device and placement == "three" and not sharded and terms.execution("marker_bary_fused")):
        if sharded:
            terms.refuse_sharded((PRIOR, POSE_ACCEL))
        return "composed"
    if sharded:
        terms.refuse_sharded((PRIOR, POSE_ACCEL))
        return "sharded"
    return "fused"


def lockstep_supported(config: Dict, stage: str) -> bool:
    """True when `stage` ("chamfer" / "marker") of this configuration runs on the fused device closure with the L-BFGS
    driver, i.e. when independent solves of it can be stepped together (engine.solve_batch): no term is on that a lock-step
    batch does not carry -- the Geman-McClure term it carries, on its fused closure -- nor the point-to-surface term or the
    per-frame vertex table, and no loss key beyond the fused closures'."""
    st = config["stages"][stage]
    if str(config["optimizer"].get("type", "lbfgs")).lower() != "lbfgs":
        return False
    terms = StageTerms(config, stage)
    if any(terms.on(t) and not (t.batch and terms.execution(t.switch)) for t in TERMS if stage in t.stages):
        return False
    if stage == "chamfer":
        return not stage_surface(config)[0] > 0.0 and not (set(st["losses"]) - stage_keys(stage) - {SURFACE_KEY}) and \
            bool(st["yaw_lock"])
    return tracklets_config(config) is None and not (set(st["losses"]) - stage_keys(stage)) and not st.get("use_sdf")
