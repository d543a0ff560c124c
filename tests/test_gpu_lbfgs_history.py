"""The three kernels that turn (history, gradient) into an L-BFGS direction -- k_lb_dots, k_lb_small_inv, k_lb_direction --
against the float64 two-loop recursion over the same window, replayed step by step with prescribed inputs through the debug
library's uuo_debug_lb_replay_* hook (csrc/solver_debug.hip): no objective, no line search, no host decision.  The
sequences (tests/lbfgs_replay.py) run past a full window: the window slides, the ring of hist + 1 slots wraps, pairs are
rejected on an empty, a partly filled, a full and a wrapped window, and the inverse factor W is the kernel's own after
hundreds of incremental column appends.  tests/test_lbfgs_replay_reference.py (CPU) checks the reference side of this.

What each case returns is recorded (record_property) and printed: the largest excess of |d - d64| over the rounding of the
fp32 store, in units of max|d64|, beside the same figure of an fp32 torch-style two-loop recursion."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_replay as lr  # noqa: E402

from gpu_support import dev  # noqa: E402,F401
from uuo_mocap_amd import _lib  # noqa: E402

LB_MAXH = 104  # csrc/lbfgs.h
HALF_ULP32 = 2.0 ** -24


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Replay:
    """One uuo_debug_lb_replay handle."""

    def __init__(self, n, hist):
        self.lib = _lib.load_debug()
        self.n = n
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.uuo_debug_lb_replay_create(n, hist, ctypes.byref(self.h)), "uuo_debug_lb_replay_create")

    def step(self, g, t_prev, t, x):
        d, xt, out = np.empty(self.n, np.float32), np.empty(self.n, np.float32), np.zeros(9)
        g, x = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(x, np.float32)
        _lib.check(self.lib.uuo_debug_lb_replay_step(self.h, _ptr(g), float(t_prev), float(t), _ptr(x), _ptr(d), _ptr(xt),
                                                     _ptr(out)), "uuo_debug_lb_replay_step")
        return d, xt, dict(gtd=out[0], accepted=out[1] != 0.0, ys=out[2], dmax=out[3], head=int(out[4]), count=int(out[5]),
                           Hdiag=out[6], host_head=int(out[7]), host_count=int(out[8]))

    def matrices(self):
        W, SY, YY = (np.empty((LB_MAXH, LB_MAXH)) for _ in range(3))
        _lib.check(self.lib.uuo_debug_lb_replay_state(self.h, _ptr(W), _ptr(SY), _ptr(YY), -1, None, None),
                   "uuo_debug_lb_replay_state")
        return W, SY, YY

    def pair(self, slot):
        s, y = np.empty(self.n, np.float32), np.empty(self.n, np.float32)
        _lib.check(self.lib.uuo_debug_lb_replay_state(self.h, None, None, None, slot, _ptr(s), _ptr(y)),
                   "uuo_debug_lb_replay_state")
        return s, y

    def close(self):
        if self.h:
            self.lib.uuo_debug_lb_replay_destroy(self.h)
            self.h = ctypes.c_void_p()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check_window_state(rep, seq, where):
    """The device's Gram copies, its carried inverse and every stored pair of the window against the host's window."""
    k = len(seq.S)
    slots = [(seq.head + j) % seq.cap for j in range(k)]
    assert slots == seq.slots, where
    for j, slot in enumerate(slots):  # a pair stays what it was for as long as it is in the window
        s, y = rep.pair(slot)
        assert _same_bits(s, seq.S[j]) and _same_bits(y, seq.Y[j]), (where, "stored pair", j, slot)
    if k == 0:
        return
    W, SY, YY = rep.matrices()
    ix = np.ix_(slots, slots)
    Sm, Ym = np.stack(seq.S64), np.stack(seq.Y64)
    sn, yn = np.linalg.norm(Sm, axis=1), np.linalg.norm(Ym, axis=1)
    # Gram copies: 1e-12 relative to the scale of each dot product, |s_i| |y_j| (Cauchy-Schwarz): the scale its fp64
    # accumulation error is proportional to -- an entry of two nearly orthogonal vectors has no relative accuracy of its own
    assert np.all(np.abs(SY[ix] - Sm @ Ym.T) <= 1e-12 * np.outer(sn, yn)), (where, "SY")
    assert np.all(np.abs(YY[ix] - Ym @ Ym.T) <= 1e-12 * np.outer(yn, yn)), (where, "YY")
    U, Wl = np.triu(SY[ix]), W[ix]
    assert np.all(np.tril(Wl, -1) == 0.0), (where, "W below the logical diagonal")
    bar = 1e-11 * np.abs(Wl).max() * np.abs(U).max()
    resid = np.abs(Wl @ U - np.eye(k)).max()
    Wh = lr.back_substitution_inverse(U)
    # W - Wh = (W U - I) Wh: the same bar, carried through the host inverse's largest entry
    gap = np.abs(Wl - Wh).max() / np.abs(Wh).max()
    print("OBS lbfgs replay %s: k %d, max|W U - I| %.2e, max|W - Wh| / max|Wh| %.2e (bar %.2e), cond(U) %.3g"
          % (where, k, resid, gap, bar, np.linalg.cond(U)))
    assert resid <= bar, (where, resid, bar)
    assert gap <= bar, (where, gap, bar)


def _run_case(case, checks=True):
    """Drives one sequence through the kernels; with `checks` every step is compared with the float64 reference.
    Returns the directions of all steps and the observed maxima."""
    n, hist, T, seed, c = case
    name = lr.case_id(case)
    seq = lr.ReplaySequence(n, hist, T, seed, c)
    rep = Replay(n, hist)
    ds, obs = [], dict(excess=0.0, err=0.0, err32=0.0, rejected=0, accepted=0)
    try:
        Hdiag_prev = 1.0
        for i in range(T):
            g, t_prev, t, x = seq.inputs()
            d, xt, out = rep.step(g, t_prev, t, x)
            ds.append(d)
            if not checks:
                if i + 1 < T:
                    seq.advance(d)
                continue
            where = "%s step %d" % (name, i)
            # ---- bookkeeping, exact
            assert (out["head"], out["count"]) == (seq.head, seq.count) == (out["host_head"], out["host_count"]), where
            if i == 0:
                assert _same_bits(d, -g), where
                assert not out["accepted"] and out["Hdiag"] == 1.0, where
            else:
                rec = seq.pushes[i - 1]
                assert out["accepted"] == rec["accepted"], (where, out["ys"], rec["ys"])
                obs["accepted" if rec["accepted"] else "rejected"] += 1
                # ---- y.s and H: the dots accumulate exact fp32 products in fp64
                assert abs(out["ys"] - rec["ys"]) <= 1e-12 * abs(rec["ys"]), (where, out["ys"], rec["ys"])
                if rec["accepted"]:
                    H = rec["ys"] / rec["yy"]
                    assert abs(out["Hdiag"] - H) <= 1e-12 * H, (where, out["Hdiag"], H)
                    # ---- the stored pair, exact: s = fl32(t_prev * d_prev) is ONE fp32 multiply and y = fl32(g - g_prev)
                    # one subtraction (the library is built with -ffp-contract=off: nothing to contract them with)
                    s_dev, y_dev = rep.pair(rec["slot"])
                    assert _same_bits(s_dev, rec["s"]), (where, "stored s")
                    assert _same_bits(y_dev, rec["y"]), (where, "stored y")
                else:
                    assert out["Hdiag"] == Hdiag_prev, (where, "H changed on a rejection")
                # ---- max|d|, exact
                assert _same_bits(np.float32(out["dmax"]), np.abs(d).max()), (where, out["dmax"], np.abs(d).max())
            Hdiag_prev = out["Hdiag"]
            # ---- the direction against the float64 two-loop recursion over the host's window
            d64 = seq.reference()
            dk = d.astype(np.float64)
            dmax64 = np.abs(d64).max()
            err = np.abs(dk - d64)
            excess = float(np.clip(err - HALF_ULP32 * np.abs(d64), 0.0, None).max() / dmax64)
            obs["excess"] = max(obs["excess"], excess)
            obs["err"] = max(obs["err"], float(err.max() / dmax64))
            d32 = lr.two_loop32(g, seq.S, seq.Y).astype(np.float64)
            obs["err32"] = max(obs["err32"], float(np.abs(d32 - d64).max() / dmax64))
            assert np.all(err <= HALF_ULP32 * np.abs(d64) + 1e-9 * dmax64), (where, excess)
            if i > 0:
                g64 = g.astype(np.float64)
                gtd64 = float(g64 @ d64)
                assert abs(out["gtd"] - gtd64) <= 1e-9 * np.linalg.norm(g64) * np.linalg.norm(d64), (where, out["gtd"], gtd64)
            # ---- the trial point: xt = fl32(x + fl32(t d)), one multiply and one add as p.add_(d, alpha=t) -- bit for bit;
            # against float64(x) + float64(t) float64(d) that is two roundings of half an ulp each, of t d and of the sum,
            # so "one ulp" is the ulp of the larger of the two (when x and t d cancel, the sum's own ulp is smaller than
            # the rounding of the product t = 0.75 needs; 1, 0.5 and 0.25 scale d exactly)
            xt64 = x.astype(np.float64) + float(t) * dk
            ulp = np.spacing(np.maximum(np.abs(float(t) * dk), np.abs(xt64)).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(xt.astype(np.float64) - xt64) <= ulp), where
            assert _same_bits(xt, x + np.float32(t) * d), where
            if hist == 100 and i == T // 2:
                _check_window_state(rep, seq, where)
            if i + 1 < T:  # (the pair that the next step pushes)
                seq.advance(d)
        if checks:
            assert obs["rejected"] == sum(not p["accepted"] for p in seq.pushes)
            _check_window_state(rep, seq, "%s end" % name)
    finally:
        rep.close()
    return ds, obs


_RESULTS = {}


def _result(case):
    if case not in _RESULTS:
        _RESULTS[case] = _run_case(case)
    return _RESULTS[case]


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_history_kernels_follow_the_float64_two_loop(dev, case, record_property):
    """Every step of every case: bookkeeping (accepted, head, count, H on a rejection, d = -g on the first step), the stored
    pair and max|d| bit for bit; y.s and H to 1e-12; g.d to 1e-9 |g| |d|; the direction element-wise within the rounding of
    its fp32 store plus 1e-9 max|d64| (the coefficients 100 x the 1e-11 that
    test_direction_coefficients_block_inverse_vs_serial holds, at window condition numbers of a few hundred); the trial
    point; at the end (and mid-way at a history of 100) the Gram copies, every stored pair and the carried inverse W."""
    ds, obs = _result(case)
    n, hist, T = case[:3]
    print("OBS lbfgs replay %s: max excess over the fp32 store's rounding %.3e of max|d64| (bar 1e-9); max|d - d64| %.3e, "
          "fp32 two-loop %.3e of max|d64|; pushes accepted %d, rejected %d"
          % (lr.case_id(case), obs["excess"], obs["err"], obs["err32"], obs["accepted"], obs["rejected"]))
    record_property("direction_excess_over_store_rounding", obs["excess"])
    record_property("direction_max_err", obs["err"])
    record_property("fp32_two_loop_max_err", obs["err32"])
    assert len(ds) == T and obs["accepted"] + obs["rejected"] == T - 1
    # fp64 accumulation: over a case the kernels are at least as close to float64 as an fp32 recursion on the same window
    assert obs["err"] <= obs["err32"], (obs["err"], obs["err32"])


def test_history_kernels_are_deterministic(dev):
    """The shipped history size, full window, ring wraps: a second run returns every direction bit for bit (the sequence
    is closed-loop, so the inputs of the second run are the first's as long as the directions are)."""
    case = next(c for c in lr.CASES if c[:3] == (1100, 100, 330))
    first, _ = _result(case)
    second, _ = _run_case(case, checks=False)
    for i, (a, b) in enumerate(zip(first, second)):
        assert _same_bits(a, b), "step %d" % i
