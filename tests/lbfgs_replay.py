"""Closed-loop input sequences for the L-BFGS history kernels and their float64 references (plain helper module: no
fixtures; used by tests/test_lbfgs_replay_reference.py on the CPU and tests/test_gpu_lbfgs_history.py on the device).

The kernels under test turn (history window, gradient) into a direction.  A window that stays well conditioned over
hundreds of pushes needs y to be roughly A s, so the gradients have to react to the direction that came back:

    A       = diag(1 + 29 i / (n - 1))
    g_0     ~ N(0, 1), fp32
    t_i     cycles through (1.0, 0.5, 0.25, 0.75)
    s_i     = fl32(t_i * d_i)                      d_i: what the direction provider returned for step i
    g_{i+1} = fl32(g_i + A s_i + c N(0, 1))        the fixed-scale drift c keeps the sequence from converging (without it
                                                   every pair soon falls under the absolute 1e-10 acceptance threshold)
    y_i     = fl32(g_{i+1} - g_i)
    the pair is accepted iff float64(y.s) > 1e-10; then H = y.s / y.y and the oldest pair leaves a full window.

At planted pushes the gradient is repeated (y = 0 and y.s = 0 exactly): the very first push (the window is empty, the
direction must stay -g with the initial H = 1), two consecutive pushes mid-way, the first push after the window has
become full, and the first push after the slot ring has wrapped (an accepted pair has gone into slot 0 a second time).
One more push, three after the mid-way pair, is a rejection of the other kind: g_{i+1} = fl32(g_i - A s_i / 64 + c N'),
N' the drift's part orthogonal to s_i, so y.s = -s.A s / 64 < 0: negative curvature with a pair that is not zero -- the
candidate slot and its Gram row receive real numbers and must then stay out of the window.

c: 0.3 was the first choice.  With g_0 ~ N(0, 1) that makes the first pairs about 30 times
longer than those of the drift-dominated state the sequence settles into, and while both kinds sit in one window the
condition number of U is 1e3 .. 1e4 (measured; tests/test_lbfgs_replay_reference.py caps it at 1e3).  c = 3 puts the two
scales within a factor of three of each other: condition numbers of at most 3e2 in every case, settling near 1.7e2 at a
full window of 100.
"""
import math

import numpy as np

T_CYCLE = (1.0, 0.5, 0.25, 0.75)
YS_MIN = 1e-10  # torch.optim.LBFGS: the pair enters the history iff y.s > 1e-10

# (n, hist, T, seed, c): T direction steps = T - 1 pushes.  Each case is named for the boundary it sits on (512-column
# blocks, 256-column strips, batches of 8 slots in 4 ranges, the 64 row owners of the dot kernel, lane + 64, a full
# shipped history with ring wraps, 32 against 33 column blocks, the fits' own 126 column blocks).
CASES = [
    (1, 1, 12, 0, 3.0), (257, 1, 12, 0, 3.0),
    (511, 2, 16, 0, 3.0), (512, 3, 20, 0, 3.0), (513, 3, 20, 0, 3.0),
    (1025, 7, 40, 0, 3.0), (1100, 16, 60, 0, 3.0), (1100, 17, 60, 0, 3.0),
    (1536, 63, 150, 0, 3.0), (1536, 64, 150, 0, 3.0), (1536, 65, 150, 0, 3.0),
    (1100, 100, 330, 0, 3.0), (2049, 100, 230, 0, 3.0),
    (16384, 5, 14, 0, 3.0), (16385, 5, 14, 0, 3.0),
    (64013, 16, 40, 0, 3.0),
]


def case_id(case):
    return "n%d-h%d-T%d" % case[:3]


def dot64(a, b):
    """Correctly rounded float64 dot product of two fp32 vectors (their products are exact in float64)."""
    return math.fsum(a.astype(np.float64) * b.astype(np.float64))


def two_loop64(g, S, Y, H):
    """The textbook two-loop recursion (what torch/optim/lbfgs.py runs) in float64; S, Y: the window, oldest first."""
    q = np.array(g, np.float64)
    S = [np.asarray(s, np.float64) for s in S]  # (no copy when the caller already holds float64)
    Y = [np.asarray(y, np.float64) for y in Y]
    k = len(S)
    rho = [1.0 / float(Y[i] @ S[i]) for i in range(k)]
    al = [0.0] * k
    for i in range(k - 1, -1, -1):
        al[i] = rho[i] * float(S[i] @ q)
        q -= al[i] * Y[i]
    r = q * H
    for i in range(k):
        be = rho[i] * float(Y[i] @ r)
        r += S[i] * (al[i] - be)
    return -r


def compact64(g, S, Y, H):
    """The compact form the kernels implement, in float64: with U the upper triangle of S Y^T, W its inverse, D its
    diagonal: al = W (-S g), cy = -H al, cs = W^T (D al + H Y g - (Y Y^T) cy), d = -H g + cy.Y + cs.S.
    Returns d and U."""
    g = np.asarray(g, np.float64)
    if not S:
        return -H * g, np.zeros((0, 0))
    Sm = np.stack([np.asarray(s, np.float64) for s in S])
    Ym = np.stack([np.asarray(y, np.float64) for y in Y])
    U = np.triu(Sm @ Ym.T)
    W = back_substitution_inverse(U)
    YY = Ym @ Ym.T
    Sg, Yg = Sm @ g, Ym @ g
    al = W @ (-Sg)
    cy = -H * al
    cs = W.T @ (np.diag(U) * al + H * Yg - YY @ cy)
    return -H * g + cy @ Ym + cs @ Sm, U


def back_substitution_inverse(U):
    """Inverse of an upper triangular matrix by back substitution (all columns at once, last row first), in float64."""
    k = U.shape[0]
    W = np.zeros((k, k))
    eye = np.eye(k)
    for r in range(k - 1, -1, -1):
        W[r] = (eye[r] - U[r, r + 1:] @ W[r + 1:]) / U[r, r]
    return W


def two_loop32(g, S, Y):
    """The two-loop recursion as torch.optim.LBFGS runs it, in fp32 with torch's own dot products and axpys
    (lbfgs.py: ro = 1 / y.s, H_diag = y.s / y.y of the newest pair, q.add_(y, alpha=-al), r.add_(s, alpha=al - be))."""
    import torch

    q = torch.from_numpy(np.asarray(g, np.float32)).neg()
    old_stps = [torch.from_numpy(np.asarray(s, np.float32)) for s in S]
    old_dirs = [torch.from_numpy(np.asarray(y, np.float32)) for y in Y]
    k = len(old_stps)
    if k == 0:
        return q.numpy()
    ro = [1.0 / old_dirs[i].dot(old_stps[i]) for i in range(k)]
    ys = old_dirs[-1].dot(old_stps[-1])
    H = ys / old_dirs[-1].dot(old_dirs[-1])
    al = [None] * k
    for i in range(k - 1, -1, -1):
        al[i] = old_stps[i].dot(q) * ro[i]
        q.add_(old_dirs[i], alpha=-float(al[i]))
    r = torch.mul(q, H)
    for i in range(k):
        be = old_dirs[i].dot(r) * ro[i]
        r.add_(old_stps[i], alpha=float(al[i] - be))
    return r.numpy()


class ReplaySequence:
    """The generator above, driven step by step.  Per step i:  g, t_prev, t, x = seq.inputs();  d = provider(...);
    d64 = seq.reference();  seq.advance(d)  -- advance forms the pair that the next step pushes."""

    def __init__(self, n, hist, T, seed=0, c=3.0):
        self.n, self.hist, self.T, self.c = n, hist, T, c
        self.cap = hist + 1
        self.rng = np.random.default_rng([seed, n, hist])
        self.rng_x = np.random.default_rng([seed, n, hist, 1])
        self.A = 1.0 + 29.0 * np.arange(n, dtype=np.float64) / max(n - 1, 1)
        self.g = self.rng.standard_normal(n).astype(np.float32)
        self.g_prev = None
        self.S, self.Y, self.slots = [], [], []  # the window, oldest first, and the slot each pair was stored in
        self.S64, self.Y64 = [], []              # the same pairs widened to float64 (exact), for the references
        self.H = 1.0
        self.head = self.count = 0  # expected bookkeeping of the kernels (ring of hist + 1 slots)
        self.i = 0
        self.accepted_total = 0
        self.pushes = []  # one record per push
        self._mid = (T - 1) // 2
        self._plant_full = self._plant_wrap = 0  # 0 not yet due, 1 due at the next push, 2 done

    def step_length(self, i):
        return np.float32(T_CYCLE[i % 4])

    def inputs(self):
        """Gradient, previous step length (the pair's s is t_prev * d_prev), first-trial step length, a fresh iterate."""
        t_prev = self.step_length(self.i - 1) if self.i > 0 else np.float32(0.0)
        x = self.rng_x.standard_normal(self.n).astype(np.float32)
        return self.g, t_prev, self.step_length(self.i), x

    def reference(self):
        return two_loop64(self.g, self.S64, self.Y64, self.H)

    @property
    def cand(self):
        return (self.head + self.count) % self.cap

    def advance(self, d):
        p = self.i  # push index
        d = np.asarray(d, np.float32)
        planted = True
        negative = p == self._mid + 3
        if p == 0 or p in (self._mid, self._mid + 1) or negative:
            pass  # (a plant that is due stays due: nothing is accepted meanwhile)
        elif self._plant_full == 1:
            self._plant_full = 2
        elif self._plant_wrap == 1:
            self._plant_wrap = 2
        else:
            planted = False
        s = self.step_length(p) * d  # fp32 multiply: exactly one rounding
        noise = self.rng.standard_normal(self.n)
        if negative:
            s64 = s.astype(np.float64)
            drift = self.c * (noise - (noise @ s64) / (s64 @ s64) * s64)  # the part of the drift orthogonal to s
            g_next = (self.g.astype(np.float64) - self.A * s64 / 64.0 + drift).astype(np.float32)
        elif planted:
            g_next = self.g.copy()
        else:
            g_next = (self.g.astype(np.float64) + self.A * s.astype(np.float64) + self.c * noise).astype(np.float32)
        y = g_next - self.g  # fp32 subtraction
        ys, yy = dot64(y, s), dot64(y, y)
        accepted = ys > YS_MIN
        rec = dict(push=p, planted=planted, negative=negative, accepted=accepted, ys=ys, yy=yy, s=s, y=y, slot=self.cand,
                   H_before=self.H)
        if accepted:
            slot = self.cand
            if len(self.S) == self.hist:
                self.S.pop(0), self.Y.pop(0), self.slots.pop(0), self.S64.pop(0), self.Y64.pop(0)
                self.head = (self.head + 1) % self.cap
            else:
                self.count += 1
            self.S.append(s), self.Y.append(y), self.slots.append(slot)
            self.S64.append(s.astype(np.float64)), self.Y64.append(y.astype(np.float64))
            self.H = ys / yy
            self.accepted_total += 1
            if self._plant_full == 0 and len(self.S) == self.hist:
                self._plant_full = 1
            elif self._plant_wrap == 0 and self._plant_full == 2 and self.accepted_total >= self.cap + 1:
                self._plant_wrap = 1
        rec.update(head=self.head, count=self.count, H=self.H)
        self.pushes.append(rec)
        self.g_prev, self.g = self.g, g_next
        self.i += 1
        return rec
