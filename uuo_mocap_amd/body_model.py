"""SMPL body-model tables: loader for a licensed ``SMPL_NEUTRAL.pkl`` and a
deterministic synthetic SMPL-shaped stand-in.

The reference builds its model with ``smplx.create("./body_models/",
model_type="smpl", gender="neutral")`` (reference utils/smpl.py:22-27).  The
licensed pickle is not redistributable and is absent from both the build
container and the GPU box, so every test and benchmark runs on
:func:`synthetic_smpl`, a table set with exactly SMPL's shapes and sparsity
structure (V=6890, J=24, 10 betas, 207 pose-blend coefficients, <=4 non-zero
skin weights per vertex, sparse row-stochastic joint regressor) generated from
an integer hash so it is bit-reproducible on any box.

Only *data* lives here; the arithmetic that consumes these tables is in
``csrc/`` (HIP) and, as the checker, ``oracle/``.
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass
from typing import Optional

import numpy as np

NUM_VERTS = 6890
NUM_JOINTS = 24
NUM_BETAS = 10
NUM_POSE_FEATS = 207  # 23 joints x 9
NUM_FACES = 13776

# SMPL kinematic tree (public smplx documentation; reference utils/smpl_utils.py:11-36 lists the joint order)
SMPL_PARENTS = np.array(
    [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], dtype=np.int64
)

SMPL_JOINT_NAMES = [
    "pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle",
    "right_ankle", "spine3", "left_foot", "right_foot", "neck", "left_collar", "right_collar", "head",
    "left_shoulder", "right_shoulder", "left_elbow", "right_elbow", "left_wrist", "right_wrist",
    "left_hand", "right_hand",
]

# smplx VertexJointSelector with VERTEX_IDS['smplh']: nose, reye, leye, rear, lear,
# LBigToe, LSmallToe, LHeel, RBigToe, RSmallToe, RHeel, then l/r x thumb,index,middle,ring,pinky tips.
SMPL_EXTRA_JOINT_VIDS = np.array(
    [332, 6260, 2800, 4071, 583,
     3216, 3226, 3387, 6617, 6624, 6787,
     2746, 2319, 2445, 2556, 2673,
     6191, 5782, 5905, 6016, 6133], dtype=np.int64
)


@dataclass
class SmplTables:
    """Host-side SMPL tables (float32 / int64 numpy), layouts as smplx holds them."""

    v_template: np.ndarray  # [V,3]
    shapedirs: np.ndarray  # [V,3,10]
    posedirs: np.ndarray  # [207, V*3]   (smplx: posedirs.reshape(V*3,207).T)
    J_regressor: np.ndarray  # [24,V]
    parents: np.ndarray  # [24] int64
    lbs_weights: np.ndarray  # [V,24]
    faces: np.ndarray  # [13776,3] int64
    extra_joint_vids: np.ndarray  # [21] int64
    name: str = "synthetic"

    def checksum(self) -> int:
        """Order-dependent 64-bit checksum of every float table (pins the generator across boxes)."""
        acc = np.uint64(0)
        for arr in (self.v_template, self.shapedirs, self.posedirs, self.J_regressor, self.lbs_weights):
            bits = np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32).astype(np.uint64).ravel()
            idx = np.arange(1, bits.size + 1, dtype=np.uint64)
            with np.errstate(over="ignore"):
                acc = acc * np.uint64(0x9E3779B97F4A7C15) + np.sum(bits * (idx | np.uint64(1)), dtype=np.uint64)
        return int(acc)


# ----------------------------------------------------------------------------------------------
# deterministic hash -> floats
# ----------------------------------------------------------------------------------------------

def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def hash_uniform(seed: int, *shape: int) -> np.ndarray:
    """float64 uniforms in [0,1) from (seed, flat index) via SplitMix64; no RNG state."""
    n = int(np.prod(shape)) if shape else 1
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = _splitmix64(idx ^ _splitmix64(np.array([seed], dtype=np.uint64)))
    u = (key >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return u.reshape(shape) if shape else u[0]


def hash_normal(seed: int, *shape: int) -> np.ndarray:
    """float64 standard normals (Box-Muller on two hash streams)."""
    u1 = hash_uniform(seed * 2 + 1, *shape)
    u2 = hash_uniform(seed * 2 + 2, *shape)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


# ----------------------------------------------------------------------------------------------
# synthetic SMPL-shaped model
# ----------------------------------------------------------------------------------------------

# nominal T-pose joint centres (metres; x lateral, y up, z forward) -- SMPL-like proportions
_NOMINAL_JOINTS = np.array([
    [0.000, 0.000, 0.000],   # pelvis
    [0.070, -0.090, 0.000],  # l hip
    [-0.070, -0.090, 0.000],  # r hip
    [0.000, 0.110, -0.020],  # spine1
    [0.100, -0.470, 0.000],  # l knee
    [-0.100, -0.470, 0.000],  # r knee
    [0.000, 0.250, 0.000],   # spine2
    [0.090, -0.870, -0.030],  # l ankle
    [-0.090, -0.870, -0.030],  # r ankle
    [0.000, 0.300, 0.020],   # spine3
    [0.110, -0.930, 0.090],  # l foot
    [-0.110, -0.930, 0.090],  # r foot
    [0.000, 0.510, -0.020],  # neck
    [0.080, 0.420, 0.000],   # l collar
    [-0.080, 0.420, 0.000],  # r collar
    [0.000, 0.580, 0.030],   # head
    [0.180, 0.450, -0.010],  # l shoulder
    [-0.180, 0.450, -0.010],  # r shoulder
    [0.440, 0.440, -0.030],  # l elbow
    [-0.440, 0.440, -0.030],  # r elbow
    [0.690, 0.450, -0.030],  # l wrist
    [-0.690, 0.450, -0.030],  # r wrist
    [0.770, 0.440, -0.040],  # l hand
    [-0.770, 0.440, -0.040],  # r hand
], dtype=np.float64)

# per-joint limb radius (m) and relative surface share
_RADIUS = np.array([0.13, 0.075, 0.075, 0.12, 0.055, 0.055, 0.125, 0.04, 0.04, 0.13, 0.035, 0.035,
                    0.055, 0.06, 0.06, 0.09, 0.05, 0.05, 0.04, 0.04, 0.03, 0.03, 0.035, 0.035])


def _segment_ends(parents: np.ndarray, joints: np.ndarray) -> np.ndarray:
    """End point of the limb segment that starts at each joint."""
    ends = np.zeros_like(joints)
    for j in range(NUM_JOINTS):
        kids = np.where(parents == j)[0]
        if len(kids) == 1:
            ends[j] = joints[kids[0]]
        elif len(kids) > 1:
            ends[j] = joints[j] + 0.6 * (joints[kids].mean(axis=0) - joints[j])
        else:  # leaves: extend along the incoming bone
            p = parents[j]
            d = joints[j] - joints[p]
            d = d / np.linalg.norm(d)
            ext = {15: 0.16, 10: 0.10, 11: 0.10, 22: 0.09, 23: 0.09}.get(j, 0.08)
            ends[j] = joints[j] + ext * d
    return ends


def _point_segment_distance(p: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """p [V,3], a/b [J,3] -> [V,J] distances to segments."""
    ab = b - a  # [J,3]
    ap = p[:, None, :] - a[None]  # [V,J,3]
    t = np.clip(np.sum(ap * ab[None], axis=-1) / np.sum(ab * ab, axis=-1)[None], 0.0, 1.0)
    closest = a[None] + t[..., None] * ab[None]
    return np.linalg.norm(p[:, None, :] - closest, axis=-1)


_SYNTH_CACHE: dict = {}


def synthetic_smpl(seed: int = 0) -> SmplTables:
    """Deterministic SMPL-shaped tables (see module docstring). Cached per seed."""
    if seed in _SYNTH_CACHE:
        return _SYNTH_CACHE[seed]
    parents = SMPL_PARENTS.copy()
    J0 = _NOMINAL_JOINTS
    ends = _segment_ends(parents, J0)
    seg_len = np.linalg.norm(ends - J0, axis=1)

    # vertices per joint ~ lateral surface area, fixed up to sum exactly to V
    area = seg_len * _RADIUS
    counts = np.floor(area / area.sum() * NUM_VERTS).astype(np.int64)
    counts = np.maximum(counts, 48)
    j = 0
    while counts.sum() != NUM_VERTS:
        step = 1 if counts.sum() < NUM_VERTS else -1
        counts[j % NUM_JOINTS] += step
        j += 1

    verts = np.zeros((NUM_VERTS, 3), dtype=np.float64)
    owner = np.zeros(NUM_VERTS, dtype=np.int64)
    faces = []
    base = 0
    for jn in range(NUM_JOINTS):
        n = int(counts[jn])
        ring = max(8, int(round(np.sqrt(n * 2.0 * np.pi * _RADIUS[jn] / max(seg_len[jn], 1e-3)))))
        ring = min(ring, n)
        rows = int(np.ceil(n / ring))
        d = ends[jn] - J0[jn]
        d = d / np.linalg.norm(d)
        ref = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
        u = np.cross(d, ref)
        u /= np.linalg.norm(u)
        w = np.cross(d, u)
        jit = hash_uniform(seed * 1000 + 10 + jn, n, 3)
        k = np.arange(n)
        r_idx = k // ring
        a_idx = k % ring
        t = (r_idx + 0.25 + 0.5 * jit[:, 0]) / rows
        theta = 2.0 * np.pi * (a_idx + 0.8 * jit[:, 1] + 0.5 * (r_idx % 2)) / ring
        # taper radius toward the segment ends so limbs close up
        taper = 0.55 + 0.45 * np.sin(np.pi * np.clip(t, 0.02, 0.98))
        rad = _RADIUS[jn] * taper * (0.92 + 0.16 * jit[:, 2])
        verts[base:base + n] = (J0[jn][None] + t[:, None] * (ends[jn] - J0[jn])[None]
                                + rad[:, None] * (np.cos(theta)[:, None] * u[None] + np.sin(theta)[:, None] * w[None]))
        owner[base:base + n] = jn
        # tube faces between consecutive rings
        for r in range(rows - 1):
            for a in range(ring):
                v00 = base + r * ring + a
                v01 = base + r * ring + (a + 1) % ring
                v10 = v00 + ring
                v11 = v01 + ring
                if v10 < base + n and v11 < base + n:
                    faces.append((v00, v01, v11))
                    faces.append((v00, v11, v10))
        base += n

    faces = np.array(faces, dtype=np.int64)
    if faces.shape[0] >= NUM_FACES:
        faces = faces[:NUM_FACES]
    else:  # pad with fan triangles so the array has SMPL's face count (faces are off the hot path)
        pad = NUM_FACES - faces.shape[0]
        k = np.arange(pad, dtype=np.int64)
        extra = np.stack([k % NUM_VERTS, (k + 1) % NUM_VERTS, (k + 2) % NUM_VERTS], axis=1)
        faces = np.concatenate([faces, extra], axis=0)

    # skin weights: <=4 non-zeros per vertex (owner + nearest segments), rows sum to 1
    dist = _point_segment_distance(verts, J0, ends)  # [V,24]
    sigma = 0.06
    score = np.exp(-(dist / sigma) ** 2)
    score[np.arange(NUM_VERTS), owner] += 1.0  # owner always dominant
    order = np.argsort(-score, axis=1, kind="stable")[:, :4]
    lbs = np.zeros((NUM_VERTS, NUM_JOINTS), dtype=np.float64)
    rows_i = np.arange(NUM_VERTS)[:, None]
    top = score[rows_i, order]
    top = np.where(top < 1e-3, 0.0, top)
    top = top / top.sum(axis=1, keepdims=True)
    lbs[rows_i, order] = top

    # joint regressor: 24 nearest vertices, positive hashed weights, row-stochastic
    Jreg = np.zeros((NUM_JOINTS, NUM_VERTS), dtype=np.float64)
    for jn in range(NUM_JOINTS):
        dj = np.linalg.norm(verts - J0[jn][None], axis=1)
        near = np.argsort(dj, kind="stable")[:24]
        wj = 0.5 + hash_uniform(seed * 1000 + 200 + jn, 24)
        Jreg[jn, near] = wj / wj.sum()

    # shape blend shapes
    S = np.zeros((NUM_VERTS, 3, NUM_BETAS), dtype=np.float64)
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    S[:, :, 0] = 0.04 * verts
    S[:, 0, 1] = 0.03 * x
    S[:, 2, 1] = 0.03 * z
    S[:, 1, 2] = 0.03 * y
    S[:, 0, 3] = 0.03 * np.sign(x) * np.maximum(np.abs(x) - 0.2, 0.0)
    om = 2.0 + 10.0 * hash_uniform(seed * 1000 + 300, NUM_BETAS, 3, 3)
    ph = 2.0 * np.pi * hash_uniform(seed * 1000 + 301, NUM_BETAS, 3)
    for c in range(4, NUM_BETAS):
        for a in range(3):
            S[:, a, c] = 0.01 * np.sin(verts @ om[c, a] + ph[c, a])

    # pose blend shapes: local to the driving joint, smooth in space
    P = np.zeros((NUM_POSE_FEATS, NUM_VERTS, 3), dtype=np.float64)
    om_p = 3.0 + 12.0 * hash_uniform(seed * 1000 + 400, NUM_POSE_FEATS, 3, 3)
    ph_p = 2.0 * np.pi * hash_uniform(seed * 1000 + 401, NUM_POSE_FEATS, 3)
    for k in range(NUM_POSE_FEATS):
        jn = k // 9 + 1
        loc = lbs[:, jn] + 0.5 * lbs[:, parents[jn]] + 0.05
        for a in range(3):
            P[k, :, a] = 0.008 * loc * np.sin(verts @ om_p[k, a] + ph_p[k, a])

    tables = SmplTables(
        v_template=verts.astype(np.float32),
        shapedirs=S.astype(np.float32),
        posedirs=P.reshape(NUM_POSE_FEATS, NUM_VERTS * 3).astype(np.float32),
        J_regressor=Jreg.astype(np.float32),
        parents=parents,
        lbs_weights=lbs.astype(np.float32),
        faces=faces,
        extra_joint_vids=SMPL_EXTRA_JOINT_VIDS.copy(),
        name="synthetic-seed%d" % seed,
    )
    _SYNTH_CACHE[seed] = tables
    return tables


# ----------------------------------------------------------------------------------------------
# licensed model loader (best effort; mirrors what smplx reads from SMPL_NEUTRAL.pkl)
# ----------------------------------------------------------------------------------------------

def sole_vertices(tables: SmplTables, per_foot: int = 3) -> np.ndarray:
    """EXTENSION: the default sole points of the floor-contact term (uuo_fit_set_floor), [2, per_foot] vertex ids (row 0 the
    left foot).  For foot s: of the vertices whose dominant joint is 10 + s, those within 10 mm of that set's rest-pose minimum
    along the model's up axis (y); of those, `per_foot` by farthest-point sampling started at the lowest.  Geometric on
    purpose: the heel and toe picks of smplx (extra_joint_vids[5:11]) are a sensible explicit choice for a real SMPL
    (unverified here: no licensed model at hand), but on the synthetic tables those ids belong to other joints."""
    from .synthetic import farthest_point_vertices

    per_foot = int(per_foot)
    if per_foot < 1:
        raise ValueError("sole_vertices: per_foot must be at least 1")
    vt = tables.v_template.astype(np.float64)
    owner = np.argmax(tables.lbs_weights, axis=1)
    out = np.zeros((2, per_foot), dtype=np.int64)
    for s in range(2):
        cand = np.where(owner == 10 + s)[0]
        if len(cand) == 0:
            raise ValueError("sole_vertices: joint %d owns no vertex" % (10 + s))
        y = vt[cand, 1]
        band = cand[y <= y.min() + 0.010]
        if len(band) < per_foot:
            raise ValueError("sole_vertices: only %d vertices within 10 mm of the sole of joint %d" % (len(band), 10 + s))
        out[s] = band[farthest_point_vertices(vt[band], per_foot, start=int(np.argmin(vt[band, 1])))]
    return out


def capsule_closest_params(a1: np.ndarray, b1: np.ndarray, a2: np.ndarray, b2: np.ndarray):
    """EXTENSION: closest-point parameters (s, t) in [0, 1] of the segments [a1, b1] and [a2, b2] (arrays [..., 3], float64),
    the routine of the self-penetration term (uuo_fit_set_capsules; Ericson, Real-Time Collision Detection 5.1.9) branch for
    branch: a segment with |b - a|^2 <= 1e-12 is a point, den = A E - b^2 <= 1e-6 A E is parallel and takes s = 0."""
    a1, b1, a2, b2 = (np.asarray(x, dtype=np.float64) for x in (a1, b1, a2, b2))
    d1, d2, r = b1 - a1, b2 - a2, a1 - a2
    A, E = (d1 * d1).sum(-1), (d2 * d2).sum(-1)
    f, c, b = (d2 * r).sum(-1), (d1 * r).sum(-1), (d1 * d2).sum(-1)
    dA, dE = A <= 1e-12, E <= 1e-12
    clamp = lambda v: np.clip(v, 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = A * E - b * b
        s = np.where(den > 1e-6 * (A * E), clamp((b * f - c * E) / den), 0.0)
        t = (b * s + f) / E
        s = np.where(t < 0.0, clamp(-c / A), np.where(t > 1.0, clamp((b - c) / A), s))
        t = clamp(t)
        s = np.where(dE, clamp(-c / A), s)
        t = np.where(dE, 0.0, t)
        t = np.where(dA, clamp(f / E), t)
        s = np.where(dA, 0.0, s)
        t = np.where(dA & dE, 0.0, t)
    return s, t


def capsule_pair_depths(joints: np.ndarray, cap_joints, cap_geom, pairs) -> np.ndarray:
    """EXTENSION: overlap depths max(r_i + r_j - d, 0) [F, P] (metres, float64) of the capsule pairs of the self-penetration
    term on joints [F, >= 24, 3]: capsule c = (u, v, alpha, beta, r) spans a = J_u + alpha (J_v - J_u) .. b = J_u + beta (J_v - J_u),
    d is the distance of the two segments (capsule_closest_params)."""
    J = np.asarray(joints, dtype=np.float64)
    cj = np.asarray(cap_joints, dtype=np.int64).reshape(-1, 2)
    cg = np.asarray(cap_geom, dtype=np.float64).reshape(-1, 3)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    e = J[:, cj[:, 1]] - J[:, cj[:, 0]]
    a = J[:, cj[:, 0]] + cg[None, :, 0:1] * e
    b = J[:, cj[:, 0]] + cg[None, :, 1:2] * e
    a1, b1, a2, b2 = a[:, pr[:, 0]], b[:, pr[:, 0]], a[:, pr[:, 1]], b[:, pr[:, 1]]
    s, t = capsule_closest_params(a1, b1, a2, b2)
    delta = (a1 + s[..., None] * (b1 - a1)) - (a2 + t[..., None] * (b2 - a2))
    d = np.sqrt((delta * delta).sum(-1))
    return np.maximum(cg[pr[:, 0], 2] + cg[pr[:, 1], 2] - d, 0.0)


#: most capsules and pairs the self-penetration term takes (uuo_fit_set_capsules; UUO_CAPS_MAXC / UUO_CAPS_MAXP of the kernel)
CAPSULES_MAX, CAPSULE_PAIRS_MAX = 32, 256


def body_capsules(tables: SmplTables, shrink: float = 0.9, rest_margin: float = 0.005):
    """EXTENSION: the default capsule set of the self-penetration term (uuo_fit_set_capsules): (cap_joints [C, 2] int32,
    cap_geom [C, 3] float32 -- alpha, beta, radius --, pairs [P, 2] int32), from the rest pose at beta = 0 in float64.
    One capsule per joint j that is the dominant skinning joint of at least one vertex (O_j those vertices).  Its line: a leaf
    joint uses (parent(j), j); any other (j, k) with k the child for which the standard deviation over O_j of the distance to
    the line J_j J_k is smallest (lowest k on ties).  alpha, beta are the 10th and 90th percentile (numpy's default
    interpolation) of the vertices' unclamped projection parameters on that line, the radius `shrink` x the median distance of
    O_j to the segment [alpha, beta].  Pairs: all i < j, except those whose joint sets share a joint or in which a joint of one
    is the parent of a joint of the other (neighbouring parts overlap by construction), and those closer than
    r_i + r_j + rest_margin in the rest pose.  More than 256 pairs is a ValueError.
    Geometric on purpose, and checked on the synthetic tables only: on a real SMPL the rule is unverified (no licensed model
    at hand).  The radii do not follow the shape parameters."""
    vt = tables.v_template.astype(np.float64)
    J = tables.J_regressor.astype(np.float64) @ vt
    parents = np.asarray(tables.parents).astype(np.int64)
    owner = np.argmax(tables.lbs_weights, axis=1)
    cj, cg = [], []
    for j in range(NUM_JOINTS):
        O = vt[owner == j]
        if len(O) == 0:
            continue
        kids = np.where(parents == j)[0]
        if len(kids) == 0:
            u, v = int(parents[j]), j
        else:
            best = None
            for k in kids:
                e = J[k] - J[j]
                t = ((O - J[j]) @ e) / (e @ e)
                sd = np.std(np.linalg.norm(O - (J[j] + t[:, None] * e), axis=1))
                if best is None or sd < best[0]:
                    best = (sd, int(k))
            u, v = j, best[1]
        e = J[v] - J[u]
        t = ((O - J[u]) @ e) / (e @ e)
        al, be = np.percentile(t, 10.0), np.percentile(t, 90.0)
        tc = np.clip(t, al, be)
        rad = float(shrink) * float(np.median(np.linalg.norm(O - (J[u] + tc[:, None] * e), axis=1)))
        cj.append((u, v))
        cg.append((al, be, rad))
    cj, cg = np.asarray(cj, dtype=np.int64), np.asarray(cg, dtype=np.float64)
    C = len(cj)
    cand = []
    for i in range(C):
        for j in range(i + 1, C):
            si, sj = set(cj[i].tolist()), set(cj[j].tolist())
            if si & sj or any(parents[q] in sj for q in si) or any(parents[q] in si for q in sj):
                continue
            cand.append((i, j))
    if cand:
        gap = capsule_pair_depths(J[None], cj, np.concatenate([cg[:, :2], cg[:, 2:] + 0.5 * float(rest_margin)], axis=1), cand)[0]
        cand = [pq for pq, g in zip(cand, gap) if not g > 0.0]  # (r_i + r_j + rest_margin - d > 0: too close at rest)
    if len(cand) > CAPSULE_PAIRS_MAX:
        raise ValueError("body_capsules: %d pairs, more than the %d the self-penetration term takes" % (len(cand), CAPSULE_PAIRS_MAX))
    return cj.astype(np.int32), cg.astype(np.float32), np.asarray(cand, dtype=np.int32).reshape(-1, 2)


#: the two thresholds of the joint-angle limit term's rotation logarithm (uuo_fit_set_joint_limits): below LIMIT_SMALL_N the axis
#: is not formed -- c >= 0 is the identity branch (kappa = 1), c < 0 a half turn that contributes nothing
LIMIT_SMALL_N = 1e-4


def rotation_log(R: np.ndarray):
    """EXTENSION: the axis-angle vector omega [..., 3] (float64) of rotations R [..., 3, 3], the host's routine of the joint-angle
    limit term (uuo_fit_set_joint_limits), branch for branch: s = 1/2 (R21 - R12, R02 - R20, R10 - R01), c = 1/2 (tr R - 1),
    n = |s|, theta = atan2(n, c), omega = (theta / n) s; n < 1e-4 and c >= 0 takes omega = s (identity branch), n < 1e-4 and
    c < 0 is a half turn, which has no axis: omega = 0 there and `skipped` is True.  Returns (omega, skipped [...])."""
    R = np.asarray(R, dtype=np.float64)
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    n = np.sqrt((s * s).sum(-1))
    small = n < LIMIT_SMALL_N
    kappa = np.where(small, 1.0, np.arctan2(n, c) / np.where(small, 1.0, n))
    skipped = small & (c < 0.0)
    return np.where(skipped[..., None], 0.0, kappa[..., None] * s), skipped


def joint_limit_violation(rot_body: np.ndarray, lo, hi) -> np.ndarray:
    """EXTENSION: pen [F, 23, 3] (radians, float64) = max(omega - hi, 0) + max(lo - omega, 0) of the joint-angle limit term on body
    rotations [F, 23, 3, 3] (rotation_log; half turns contribute nothing)."""
    om, skipped = rotation_log(rot_body)
    lo = np.asarray(lo, dtype=np.float64).reshape(23, 3)
    hi = np.asarray(hi, dtype=np.float64).reshape(23, 3)
    pen = np.maximum(om - hi, 0.0) + np.maximum(lo - om, 0.0)
    return np.where(skipped[..., None], 0.0, pen)


def smpl_joint_limits(flex: float = 2.70, slack: float = 0.10):
    """EXTENSION: the default tables of the joint-angle limit term (uuo_fit_set_joint_limits): (lo, hi), float32 [23, 3] in
    radians on the components of each body joint's axis-angle vector (row j - 1 is SMPL joint j), infinite except SMPLify's
    four hinge components: knees (joints 4, 5) x in [-slack, flex], left elbow (18) y in [-flex, slack], right elbow (19) y in
    [-slack, flex].  The signs are those of SMPLify's angle prior; synthetic_smpl uses SMPL's nominal y-up rest joints, so they
    hold for it too.  flex (about 155 degrees of flexion) and slack (about 6 degrees of hyperextension) are an anatomical choice,
    a parameter, not a measurement; on a licensed SMPL they are unverified (no licensed model at hand)."""
    flex, slack = float(flex), float(slack)
    if not (np.isfinite(flex) and np.isfinite(slack) and flex >= 0.0 and slack >= 0.0):
        raise ValueError("smpl_joint_limits: flex and slack are non-negative finite angles in radians")
    lo = np.full((23, 3), -np.inf, dtype=np.float32)
    hi = np.full((23, 3), np.inf, dtype=np.float32)
    for j in (4, 5):
        lo[j - 1, 0], hi[j - 1, 0] = -slack, flex
    lo[18 - 1, 1], hi[18 - 1, 1] = -flex, slack
    lo[19 - 1, 1], hi[19 - 1, 1] = -slack, flex
    return lo, hi


#: most components the mixture pose prior takes (uuo_fit_set_pose_gmm), and the length of its pose vector
POSE_MIXTURE_MAX = 16
POSE_MIXTURE_DIM = 69


def pose_log_vector(rot_body: np.ndarray) -> np.ndarray:
    """EXTENSION: theta [F, 69] (float64) of the mixture pose prior (uuo_fit_set_pose_gmm): the concatenation of the 23 body
    joints' axis-angle vectors of rot_body [F, 23, 3, 3] (rotation_log: a half turn contributes zeros)."""
    om, _ = rotation_log(np.asarray(rot_body, dtype=np.float64).reshape(-1, 23, 3, 3))
    return om.reshape(-1, POSE_MIXTURE_DIM)


def check_pose_mixture(means, covars, weights, what: str = "pose mixture"):
    """(means [K, 69], covars [K, 69, 69], weights [K] summing to 1) in float64, or a ValueError that names `what` and the fault:
    the shapes, 1 <= K <= 16, finiteness, positive weights, symmetry to 1e-6 relative, positive definiteness (Cholesky)."""
    try:
        mu, cov, pi = (np.asarray(a, dtype=np.float64) for a in (means, covars, weights))
    except (TypeError, ValueError):
        raise ValueError("%s: means, covars and weights must be numeric arrays" % what)
    K = mu.shape[0] if mu.ndim == 2 else -1
    if mu.ndim != 2 or mu.shape[1] != POSE_MIXTURE_DIM or cov.shape != (K, POSE_MIXTURE_DIM, POSE_MIXTURE_DIM) or pi.shape != (K,):
        raise ValueError("%s: means [K, 69], covars [K, 69, 69] and weights [K] expected (got %s, %s, %s)"
                         % (what, mu.shape, cov.shape, pi.shape))
    if not 1 <= K <= POSE_MIXTURE_MAX:
        raise ValueError("%s: 1 .. %d components expected (got %d)" % (what, POSE_MIXTURE_MAX, K))
    if not (np.isfinite(mu).all() and np.isfinite(cov).all() and np.isfinite(pi).all()):
        raise ValueError("%s: a non-finite entry" % what)
    if not (pi > 0.0).all():
        raise ValueError("%s: the weights must be positive" % what)
    for k in range(K):
        if np.abs(cov[k] - cov[k].T).max() > 1e-6 * np.abs(cov[k]).max():
            raise ValueError("%s: the covariance of component %d is not symmetric (to 1e-6 relative)" % (what, k))
        try:
            np.linalg.cholesky(0.5 * (cov[k] + cov[k].T))
        except np.linalg.LinAlgError:
            raise ValueError("%s: the covariance of component %d is not positive definite" % (what, k))
    return mu, cov, pi / pi.sum()


def load_pose_mixture(path: str):
    """EXTENSION: a Gaussian mixture over the 69 axis-angle components of the body pose -- {"means" [K, 69], "covars"
    [K, 69, 69], "weights" [K]} in float64, the weights renormalised -- from an .npz with these keys or a SMPLify-style pickle (a
    dict with the same keys, read with encoding="latin1": SMPLify's gmm_08.pkl).  Checked by check_pose_mixture; every error is a
    ValueError that names the file and the fault."""
    what = "load_pose_mixture(%s)" % path
    try:
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as fh:
                data = {k: fh[k] for k in fh.files}
        else:
            with open(path, "rb") as fh:
                data = pickle.load(fh, encoding="latin1")
    except Exception as e:  # (whatever a damaged archive or a pickle that names a missing module or attribute raises: BadZipFile,
        # ImportError, AttributeError, ... -- every fault of the file leaves here as a ValueError that names it)
        raise ValueError("%s: cannot be read (%s: %s)" % (what, type(e).__name__, e))
    if not isinstance(data, dict) or not {"means", "covars", "weights"} <= set(data):
        raise ValueError("%s: the keys means, covars and weights expected (got %s)"
                         % (what, sorted(data) if isinstance(data, dict) else type(data).__name__))
    mu, cov, pi = check_pose_mixture(data["means"], data["covars"], data["weights"], what)
    return {"means": mu, "covars": cov, "weights": pi}


def prepare_pose_mixture(means, covars, weights):
    """EXTENSION: the mixture as uuo_fit_set_pose_gmm and losses.pose_gmm_loss take it -- float32 (means [K, 69], chol [K, 69, 69],
    offsets [K]) from float64: chol[k] = A_k lower triangular with A_k A_k^T = Sigma_k^-1 (the Cholesky factor of the inverse),
    offsets[k] = -log pi_k + 1/2 log det Sigma_k, shifted so that the least is 0 (SMPLify's constant up to a shift: the shift
    moves the loss by a constant and no gradient).  Checked by check_pose_mixture first."""
    mu, cov, pi = check_pose_mixture(means, covars, weights, "prepare_pose_mixture")
    mu, chol, offsets = pose_mixture_factors(mu, cov, pi)
    return (np.ascontiguousarray(mu, dtype=np.float32), np.ascontiguousarray(chol, dtype=np.float32),
            np.ascontiguousarray(offsets, dtype=np.float32))


def pose_mixture_factors(mu: np.ndarray, cov: np.ndarray, pi: np.ndarray):
    """prepare_pose_mixture's arithmetic in float64, unchecked: (means, A_k, offsets)."""
    K = mu.shape[0]
    chol = np.zeros_like(cov)
    offsets = np.zeros(K)
    for k in range(K):
        sym = 0.5 * (cov[k] + cov[k].T)
        chol[k] = np.linalg.cholesky(np.linalg.inv(sym))
        offsets[k] = -np.log(pi[k]) + 0.5 * np.linalg.slogdet(sym)[1]
    return mu, chol, offsets - offsets.min()


class _ChStub:
    """Stands in for chumpy.ch.Ch when unpickling original SMPL files (install.sh:18 needs chumpy)."""

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {})

    @property
    def r(self):
        return np.asarray(self.__dict__.get("x"))


class _SmplUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("chumpy"):
            return _ChStub
        return super().find_class(module, name)


def _to_np(x):
    if isinstance(x, _ChStub):
        return np.asarray(x.r)
    if hasattr(x, "toarray"):
        return np.asarray(x.toarray())
    return np.asarray(x)


def load_smpl_pkl(path: str) -> SmplTables:
    with open(path, "rb") as fh:
        data = _SmplUnpickler(fh, encoding="latin1").load()
    v_t = _to_np(data["v_template"]).astype(np.float32)
    V = v_t.shape[0]
    shapedirs = _to_np(data["shapedirs"])[:, :, :NUM_BETAS].astype(np.float32)
    posedirs = _to_np(data["posedirs"]).astype(np.float32)  # [V,3,207]
    posedirs = posedirs.reshape(V * 3, -1).T.copy()
    kintree = _to_np(data["kintree_table"]).astype(np.int64)
    parents = kintree[0].copy()
    parents[0] = -1
    return SmplTables(
        v_template=v_t,
        shapedirs=shapedirs,
        posedirs=posedirs,
        J_regressor=_to_np(data["J_regressor"]).astype(np.float32),
        parents=parents,
        lbs_weights=_to_np(data["weights"]).astype(np.float32),
        faces=_to_np(data["f"]).astype(np.int64),
        extra_joint_vids=SMPL_EXTRA_JOINT_VIDS.copy(),
        name=os.path.basename(path),
    )


def load_model(body_model_path: str = "./body_models/", gender: str = "neutral",
               allow_synthetic: bool = True) -> SmplTables:
    """smplx.create(path, model_type="smpl", gender=...) equivalent: real pickle iff present."""
    fn = os.path.join(body_model_path, "smpl", "SMPL_%s.pkl" % gender.upper())
    if os.path.isfile(fn):
        return load_smpl_pkl(fn)
    if not allow_synthetic:
        raise FileNotFoundError(fn)
    return synthetic_smpl(0)
