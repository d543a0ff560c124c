"""A heavy-tailed, SMPL-scale stress model and stress inputs for the kernels' float64 tests (a plain helper module, imported
by tests/test_model_range.py and tests/test_gpu_model_range.py the way tests/converged_records.py is).

Every other test runs on ``synthetic_smpl(0)``, whose blend bases are small and smooth (posedirs < 0.0084 m, shapedirs
< 0.040 m), whose smallest non-zero skin weight is 4e-4 and whose joint-regressor rows hold 24 entries.  The product is
meant to run the licensed ``SMPL_NEUTRAL.pkl``, which is not available to this suite, so the real model's statistics are
NOT known here.  The targets below are assumptions chosen to cover them with margin:

* ``posedirs`` and ``shapedirs``: random-sign entries, log-uniform magnitudes over 1e-7 .. 1e-1 m on the vertices the
  driving joint (or its parent) skins, 1e-10 .. 1e-4 m elsewhere with about a third exact zeros, a few entries of
  0.1 .. 0.15 m in each basis, and a ``shapedirs[..., 0]`` column that scales the body by 0.12 m per unit beta with a
  few entries of about 0.2 m.  After k_skin3's power-of-two scale (csrc/model.hip) many entries sit where the fp16 lo
  plane is subnormal (scaled value < 2^-3) and some where the hi plane is too (< 2^-14).
* skin weights: at most 4 non-zeros per vertex (what ``uuo_model_create`` accepts); most vertices have exactly 4, the
  extra three drawn log-uniform over 1e-5 .. 0.5 of the owner's weight, so weights go down to about 1e-5; rows sum to 1 in
  float64, not exactly in float32.
* ``J_regressor``: non-negative, row-stochastic, 100 .. 300 non-zeros per row on the vertices nearest the joint.

Topology and template (V = 6890, 13 776 faces, SMPL's parents) are those of ``synthetic_smpl(seed)``.  The tables are
returned in ``SMPL_NEUTRAL.pkl`` layout (float64, scipy-sparse ``J_regressor``, ``[V, 3, 207]`` posedirs, uint32
``kintree_table``) so that tests load them back through ``body_model.load_smpl_pkl``.
"""
from __future__ import annotations

import functools
import pickle

import numpy as np

from uuo_mocap_amd.body_model import (NUM_BETAS, NUM_JOINTS, NUM_POSE_FEATS, NUM_VERTS, hash_uniform, load_smpl_pkl,
                                      synthetic_smpl)

BIG_POSEDIRS = 12    # posedirs entries of 0.1 .. 0.15 m
BIG_SHAPEDIRS = 12   # shapedirs entries of 0.1 .. 0.2 m (columns 1..9) and as many of 0.15 .. 0.2 m in column 0
FOLD = np.pi - 0.3   # bend of the folded joints

# joints folded in the "folded" frames, with the axis each one bends about (SMPL: x lateral, y up, z forward)
_FOLDS = ((1, 0), (2, 0), (4, 0), (5, 0), (16, 2), (17, 2), (18, 1), (19, 1))


def _log_uniform(seed, shape, lo_exp, hi_exp):
    return 10.0 ** (lo_exp + (hi_exp - lo_exp) * hash_uniform(seed, *shape))


def _sign(seed, shape):
    return np.where(hash_uniform(seed, *shape) < 0.5, -1.0, 1.0)


def _heavy_basis(seed, near):
    """Random-sign, heavy-tailed entries: log-uniform 1e-7 .. 1e-1 where `near`, 1e-10 .. 1e-4 (a third zeros) elsewhere."""
    shape = near.shape
    mag = np.where(near, _log_uniform(seed, shape, -7.0, -1.0), _log_uniform(seed + 1, shape, -10.0, -4.0))
    mag = np.where(~near & (hash_uniform(seed + 2, *shape) < 1.0 / 3.0), 0.0, mag)
    return _sign(seed + 3, shape) * mag


def _set_big(arr, seed, count, lo, hi, allowed):
    """Sets `count` entries of `arr` (where `allowed`) to random-sign magnitudes uniform in [lo, hi]."""
    cand = np.flatnonzero(allowed.reshape(-1))
    pick = cand[np.argsort(hash_uniform(seed, cand.size), kind="stable")[:count]]
    flat = arr.reshape(-1)
    flat[pick] = _sign(seed + 1, (count,)) * (lo + (hi - lo) * hash_uniform(seed + 2, count))


@functools.lru_cache(maxsize=4)
def heavy_smpl(seed: int = 0) -> dict:
    """The stress model as the dict that ``SMPL_NEUTRAL.pkl`` holds (float64 arrays; see the module docstring).  Cached:
    treat the returned arrays as read-only."""
    base = synthetic_smpl(seed)
    s = 7001 * (seed + 1)
    V, J = NUM_VERTS, NUM_JOINTS
    vt = base.v_template.astype(np.float64)
    parents = np.asarray(base.parents, np.int64)
    owner_w = base.lbs_weights.astype(np.float64)  # the synthetic model's skinning: which joints a vertex belongs to

    # pose blend shapes [207, V, 3]: local to the driving joint (feature k drives joint k // 9 + 1) and its parent
    jn = np.arange(NUM_POSE_FEATS) // 9 + 1
    near_p = (owner_w[:, jn] + owner_w[:, parents[jn]]).T > 0.0  # [207, V]
    P = _heavy_basis(s + 10, np.repeat(near_p[:, :, None], 3, axis=2))
    _set_big(P, s + 20, BIG_POSEDIRS, 0.10, 0.15, np.repeat(near_p[:, :, None], 3, axis=2))

    # shape blend shapes [V, 3, 10]: column 0 scales the body (0.12 m per unit beta per metre from the pelvis), all columns
    # carry the heavy tail; columns 1..9 are local to a random joint each
    near_s = np.zeros((V, 3, NUM_BETAS), dtype=bool)
    near_s[:, :, 0] = True
    cj = (hash_uniform(s + 30, NUM_BETAS) * J).astype(np.int64)
    for c in range(1, NUM_BETAS):
        near_s[:, :, c] = (owner_w[:, cj[c]] + owner_w[:, parents[cj[c]] if cj[c] > 0 else 0] > 0.0)[:, None]
    S = _heavy_basis(s + 40, near_s)
    S[:, :, 0] += 0.12 * vt
    col0 = np.zeros_like(near_s)
    col0[:, :, 0] = True
    _set_big(S, s + 50, BIG_SHAPEDIRS, 0.15, 0.20, col0)
    _set_big(S, s + 60, BIG_SHAPEDIRS, 0.10, 0.20, near_s & ~col0)

    # skin weights: the synthetic model's joints of each vertex, completed to four by the nearest other joints; the
    # owner keeps weight 1 before normalisation, the others are log-uniform in 1e-5 .. 0.5 (some vertices keep 2 or 3)
    J0 = base.J_regressor.astype(np.float64) @ vt
    d = np.linalg.norm(vt[:, None, :] - J0[None], axis=-1)  # [V, J]
    owner = np.argmax(owner_w, axis=1)
    d[np.arange(V), owner] = -1.0
    order = np.argsort(d, axis=1, kind="stable")[:, :4]  # owner first, then the three nearest joints
    w = np.empty((V, 4))
    w[:, 0] = 1.0
    w[:, 1:] = _log_uniform(s + 70, (V, 3), -5.0, np.log10(0.5))
    u = hash_uniform(s + 71, V)
    w[u < 0.08, 3] = 0.0  # 8 % of the vertices with at most three joints ...
    w[u < 0.02, 2] = 0.0  # ... 2 % with at most two
    w /= w.sum(axis=1, keepdims=True)
    lbs = np.zeros((V, J))
    lbs[np.arange(V)[:, None], order] = w

    # joint regressor: 100 .. 300 nearest vertices per joint, positive weights spread over two decades, row-stochastic
    Jreg = np.zeros((J, V))
    nnz = 100 + (hash_uniform(s + 80, J) * 201).astype(np.int64)
    for j in range(J):
        near = np.argsort(np.linalg.norm(vt - J0[j][None], axis=1), kind="stable")[:nnz[j]]
        wj = _log_uniform(s + 81 + j, (int(nnz[j]),), -2.0, 0.0)
        Jreg[j, near] = wj / wj.sum()

    import scipy.sparse as sp

    kintree = np.stack([parents, np.arange(J, dtype=np.int64)]).astype(np.uint32)
    kintree[0, 0] = 4294967295
    return {
        "v_template": vt,
        "shapedirs": S,
        "posedirs": np.ascontiguousarray(P.transpose(1, 2, 0)),  # [V, 3, 207]
        "J_regressor": sp.csc_matrix(Jreg),
        "weights": lbs,
        "kintree_table": kintree,
        "f": np.asarray(base.faces, np.uint32),
        "bs_type": "lrotmin", "bs_style": "lbs",
    }


def write_pkl(path: str, seed: int = 0) -> str:
    """Writes ``heavy_smpl(seed)`` as a latin1-readable protocol-2 pickle (the layout of SMPL_NEUTRAL.pkl)."""
    with open(path, "wb") as fh:
        pickle.dump(heavy_smpl(seed), fh, protocol=2)
    return path


def load(path: str):
    """The stress model as the product reads it (float32 SmplTables through body_model.load_smpl_pkl)."""
    return load_smpl_pkl(path)


def skin16_scale(tables) -> float:
    """k_skin3's power of two for the [posedirs | shapedirs] basis (csrc/model.hip): brings the largest |entry| into
    [128, 256)."""
    amax = max(float(np.abs(tables.posedirs).max()), float(np.abs(tables.shapedirs).max()))
    _, e = np.frexp(np.float32(amax))
    return float(np.ldexp(1.0, 8 - int(e)))


# ------------------------------------------------------------------------------------------------ stress inputs
def _rot(axis_angle):
    """Rodrigues in float64: [..., 3] -> [..., 3, 3]."""
    th = np.linalg.norm(axis_angle, axis=-1, keepdims=True)
    k = axis_angle / np.maximum(th, 1e-300)
    K = np.zeros(axis_angle.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -k[..., 2], k[..., 1], -k[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = k[..., 2], -k[..., 1], k[..., 0]
    th = th[..., None]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def frame_kinds(F: int) -> np.ndarray:
    """0 identity, 1 folded, 2 random full-range rotations (the folded and random kinds alternate; every 7th frame is
    the identity)."""
    f = np.arange(F)
    return np.where(f % 7 == 3, 0, np.where(f % 2 == 0, 1, 2))


def stress_inputs(F: int, seed: int = 0) -> dict:
    """Float32 inputs of the stress tests (numpy): `pose` [F, 23, 3, 3] -- per frame the identity, a "folded" pose
    (hips, knees, shoulders and elbows bent by about pi - 0.3 either way, plus 0.1 rad of jitter on every joint) or random
    full-range rotations --, `root` [F, 1, 3, 3] (random, identity on identity frames), `z` [F, 1, 1] in [-pi, pi),
    `betas` [1, 10] and `betas_f` [F, 10] uniform in [-5, 5], `trans` [F, 3] uniform in [-3, 3] m."""
    s = 9173 * (seed + 1)
    kind = frame_kinds(F)
    aa = np.zeros((F, NUM_JOINTS, 3))
    rnd_axis = 2.0 * hash_uniform(s + 1, F, NUM_JOINTS, 3) - 1.0
    rnd_axis /= np.linalg.norm(rnd_axis, axis=-1, keepdims=True)
    rnd = rnd_axis * (np.pi * hash_uniform(s + 2, F, NUM_JOINTS, 1))
    jitter = 0.1 * (2.0 * hash_uniform(s + 3, F, NUM_JOINTS, 3) - 1.0)
    fold = jitter.copy()
    sgn = _sign(s + 4, (F, len(_FOLDS)))
    for i, (j, ax) in enumerate(_FOLDS):
        fold[:, j, ax] += sgn[:, i] * FOLD
    aa[kind == 1] = fold[kind == 1]
    aa[kind == 2] = rnd[kind == 2]
    aa[kind == 1, 0] = rnd[kind == 1, 0]  # folded frames keep a random root
    R = _rot(aa)
    R[kind == 0] = np.eye(3)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {
        "pose": f32(R[:, 1:]),
        "root": f32(R[:, :1]),
        "z": f32(np.pi * (2.0 * hash_uniform(s + 5, F, 1, 1) - 1.0)),
        "betas": f32(10.0 * hash_uniform(s + 6, 1, NUM_BETAS) - 5.0),
        "betas_f": f32(10.0 * hash_uniform(s + 7, F, NUM_BETAS) - 5.0),
        "trans": f32(6.0 * hash_uniform(s + 8, F, 3) - 3.0),
        "kind": kind,
    }


def forward_error(tables, inp: dict, frames_per_block: int = 50):
    """Max |error| of the CPU float32 oracle's vertices and 45 joints against the float64 oracle (oracle/smpl_ref.py) at
    `inp` (per-frame betas): the float32 round-off level on the stress model."""
    import torch

    from oracle.smpl_ref import SmplInferenceRef

    r32 = SmplInferenceRef(tables)
    r64 = SmplInferenceRef(tables).double()
    F = inp["pose"].shape[0]
    ev = ej = 0.0
    with torch.no_grad():
        for a in range(0, F, frames_per_block):
            sl = slice(a, min(F, a + frames_per_block))
            args = [torch.from_numpy(inp[k][sl]) for k in ("pose", "betas_f", "root", "trans")]
            o32 = r32(*args)
            o64 = r64(*[t.double() for t in args])
            ev = max(ev, float((o32["vertices"].double() - o64["vertices"]).abs().max()))
            ej = max(ej, float((o32["joints"].double() - o64["joints"]).abs().max()))
    return ev, ej
