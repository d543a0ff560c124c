"""Float64 restatement of the mixture pose prior (uuo_fit_set_pose_gmm, losses.pose_gmm_loss) with explicit loops, and the
host-side builders the CPU and GPU tests share: rotations, the stage's Gram-Schmidt map, the two mixture recipes and poses
planted on their components.  numpy only."""
import math

import numpy as np


def rodrigues(v):
    """axis-angle -> rotation, plain float64"""
    v = np.asarray(v, dtype=np.float64)
    th = float(np.sqrt(v @ v))
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def gs64(raw):
    """the stage's normalisation (Gram-Schmidt on rows 0, 1; row 2 their cross product) on raw [..., 3, 3], float64"""
    a1, a2 = raw[..., 0, :], raw[..., 1, :]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), 1e-12)
    u2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = u2 / np.maximum(np.linalg.norm(u2, axis=-1, keepdims=True), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-2)


def term_np(R, means, chol, offsets, w):
    """loss, d loss / d R [F, 23, 3, 3], one tag per (frame, joint), the winner per frame and the energies [F, K]: the
    formulas of the term, loop by loop.  means [K, 69], chol [K, 69, 69] (lower), offsets [K], all float64."""
    R = np.asarray(R, dtype=np.float64)
    F, K = R.shape[0], means.shape[0]
    loss, g, tags, winners, energies = 0.0, np.zeros_like(R), [], [], np.zeros((F, K))
    for f in range(F):
        theta = np.zeros(69)
        parts = []
        for j in range(23):
            r = R[f, j]
            s = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
            c = 0.5 * (r[0, 0] + r[1, 1] + r[2, 2] - 1.0)
            n = math.sqrt(s @ s)
            if n < 1e-4 and c < 0.0:
                tags.append("half turn")
                parts.append(None)
                continue
            if n < 1e-4:
                kappa, dkn, dkc = 1.0, 0.0, 0.0
                tags.append("identity")
            else:
                th = math.atan2(n, c)
                kappa = th / n
                dkn = c / (n * (n * n + c * c)) - th / (n * n)
                dkc = -1.0 / (n * n + c * c)
                tags.append("generic")
            theta[3 * j:3 * j + 3] = kappa * s
            parts.append((s, n, kappa, dkn, dkc))
        best, e_best, y_best = -1, 0.0, None
        for k in range(K):
            d = theta - means[k]
            y = np.zeros(69)
            for col in range(69):   # y = A_k^T d: column col of the lower triangle against d[col:]
                y[col] = float(chol[k, col:, col] @ d[col:])
            e = 0.5 * float(y @ y) + offsets[k]
            energies[f, k] = e
            if best < 0 or e < e_best:  # (strict: ties keep the lowest k)
                best, e_best, y_best = k, e, y
        winners.append(best)
        loss += w * e_best / F
        gth = np.zeros(69)
        for row in range(69):       # A_k* y: row `row` of the lower triangle against y[:row + 1]
            gth[row] = (w / F) * float(chol[best, row, :row + 1] @ y_best[:row + 1])
        for j in range(23):
            if parts[j] is None:
                continue
            s, n, kappa, dkn, dkc = parts[j]
            gom = gth[3 * j:3 * j + 3]
            q = float(s @ gom)
            ds = kappa * gom + (q * dkn / n) * s if n >= 1e-4 else gom.copy()
            dc = q * dkc
            g[f, j, 2, 1] += 0.5 * ds[0]
            g[f, j, 1, 2] -= 0.5 * ds[0]
            g[f, j, 0, 2] += 0.5 * ds[1]
            g[f, j, 2, 0] -= 0.5 * ds[1]
            g[f, j, 1, 0] += 0.5 * ds[2]
            g[f, j, 0, 1] -= 0.5 * ds[2]
            for k in range(3):
                g[f, j, k, k] += 0.5 * dc
    return loss, g, tags, np.asarray(winners), energies


def energies_np(theta, means, chol, offsets):
    """e [F, K] of pose vectors theta [F, 69] (vectorised; for the preconditions of the GPU cases)"""
    y = np.einsum("krc,fkr->fkc", np.tril(chol), theta[:, None, :] - means[None])
    return 0.5 * (y * y).sum(-1) + offsets[None]


def _random_rotation(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))[None, :]


def make_mixture(kind, K, rng):
    """The two recipes of the GPU tests, float64 {means, covars, weights}.  "far": means 0.3 N(0, 1), covariance eigenvalues
    log-uniform in [0.02^2, 0.5^2] rad^2 (both ends taken: condition number 625) under a random rotation, equal weights.
    "close": means 0.06 N(0, 1), eigenvalues log-uniform in [0.15^2, 0.5^2], Dirichlet(8) weights."""
    lo, hi, scale = {"far": (0.02, 0.5, 0.3), "close": (0.15, 0.5, 0.06)}[kind]
    means = scale * rng.standard_normal((K, 69))
    covars = np.zeros((K, 69, 69))
    for k in range(K):
        ev = np.exp(rng.uniform(2.0 * math.log(lo), 2.0 * math.log(hi), size=69))
        ev[0], ev[1] = lo * lo, hi * hi
        Q = _random_rotation(rng, 69)
        covars[k] = (Q * ev[None, :]) @ Q.T
        covars[k] = 0.5 * (covars[k] + covars[k].T)
    weights = np.full(K, 1.0 / K) if kind == "far" else rng.dirichlet(np.full(K, 8.0))
    return {"means": means, "covars": covars, "weights": weights}


def planted_theta(mix, F, rng):
    """theta_t = mu_{t mod K} + chol(Sigma_{t mod K}) N(0, 1), [F, 69]"""
    K = mix["means"].shape[0]
    out = np.zeros((F, 69))
    for t in range(F):
        k = t % K
        out[t] = mix["means"][k] + np.linalg.cholesky(mix["covars"][k]) @ rng.standard_normal(69)
    return out


def raw_from_theta(theta, rng=None):
    """raw body pose entries [F, 23, 3, 3] whose Gram-Schmidt is the rotation of theta's joints; with `rng` the first two rows
    are scaled and sheared (raw is then not orthonormal, its third row still the rotation's)"""
    F = theta.shape[0]
    R = np.stack([np.stack([rodrigues(theta[f, 3 * j:3 * j + 3]) for j in range(23)]) for f in range(F)])
    if rng is None:
        return R
    raw = R.copy()
    a = rng.uniform(0.8, 1.25, size=(F, 23, 1))
    b = rng.uniform(0.8, 1.25, size=(F, 23, 1))
    sh = 0.1 * rng.standard_normal((F, 23, 1))
    raw[:, :, 0] = a * R[:, :, 0]
    raw[:, :, 1] = b * R[:, :, 1] + sh * R[:, :, 0]
    return raw


def find_case(kind, K, F, seed0=0, tries=200):
    """(mixture, theta [F, 69], seed) of the first seed >= seed0 that meets the GPU tests' preconditions in float64: in every
    frame the second-best energy at least 1e-2 relative above the best (K > 1), the winners over the frames min(F, K) distinct
    components and the planted ones, every joint's angle in [1e-2, 2.9]."""
    from uuo_mocap_amd.body_model import pose_mixture_factors

    for seed in range(seed0, seed0 + tries):
        rng = np.random.default_rng(seed)
        mix = make_mixture(kind, K, rng)
        theta = planted_theta(mix, F, rng)
        ang = np.linalg.norm(theta.reshape(F, 23, 3), axis=-1)
        if ang.min() < 1e-2 or ang.max() > 2.9:
            continue
        mu, chol, off = pose_mixture_factors(mix["means"], mix["covars"], mix["weights"] / mix["weights"].sum())
        e = energies_np(theta, mu, chol, off)
        win = e.argmin(axis=1)
        if not np.array_equal(win, np.arange(F) % K) or len(set(win.tolist())) != min(F, K):
            continue
        if K > 1:
            srt = np.sort(e, axis=1)
            if ((srt[:, 1] - srt[:, 0]) < 1e-2 * np.maximum(np.abs(srt[:, 0]), 1e-300)).any():
                continue
        return mix, theta, seed
    raise AssertionError("no seed in %d .. %d meets the preconditions (%s, K = %d, F = %d)" % (seed0, seed0 + tries, kind, K, F))
