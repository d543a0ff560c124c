"""Keeps tests/test_gpu_lbfgs_history.py honest about its own reference (CPU only): the closed-loop sequences of
tests/lbfgs_replay.py, fed with the float64 two-loop recursion's own output rounded to fp32, must give windows on which
the comparison means something -- the compact form the kernels implement agrees with the textbook recursion to fp64
round-off, the triangular factor stays well conditioned, the planted rejections are rejections and the natural ones rare."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_replay as lr  # noqa: E402

CPU_CASES = [c for c in lr.CASES if c[0] <= 2049]


def run_reference_loop(case):
    n, hist, T, seed, c = case
    seq = lr.ReplaySequence(n, hist, T, seed, c)
    worst_gap, worst_cond = 0.0, 1.0
    for _ in range(T):
        seq.inputs()
        d64 = seq.reference()
        dc, U = lr.compact64(seq.g, seq.S64, seq.Y64, seq.H)
        worst_gap = max(worst_gap, float(np.abs(dc - d64).max() / np.abs(d64).max()))
        if U.shape[0]:
            worst_cond = max(worst_cond, float(np.linalg.cond(U)))
        seq.advance(d64.astype(np.float32))
    return seq, worst_gap, worst_cond


@pytest.mark.parametrize("case", CPU_CASES, ids=lr.case_id)
def test_replay_sequences_are_a_sound_reference(case):
    n, hist, T, seed, c = case
    seq, worst_gap, worst_cond = run_reference_loop(case)
    pushes = seq.pushes[:T - 1]  # the last advance forms a pair that no step pushes
    planted = [p for p in pushes if p["planted"]]
    natural = [p for p in pushes if not p["planted"] and not p["accepted"]]
    print("OBS replay reference %s: compact vs two-loop %.2e of max|d|, max cond(U) %.3g, planted %d, natural rejections %d "
          "of %d pushes, accepted %d" % (lr.case_id(case), worst_gap, worst_cond, len(planted), len(natural), len(pushes),
                                        sum(p["accepted"] for p in pushes)))
    assert worst_gap <= 1e-12
    assert worst_cond <= 1e3
    assert all(not p["accepted"] and (p["ys"] < 0.0 and np.any(p["y"] != 0) if p["negative"] else p["ys"] == 0.0)
               for p in planted)
    assert sum(p["negative"] for p in planted) == 1
    assert len(natural) <= 0.15 * len(pushes)
    # the planted situations are really there: the first push, two consecutive ones, one on a full window, one after the
    # ring of hist + 1 slots has wrapped
    assert pushes[0]["planted"]
    ids = [p["push"] for p in planted]
    assert any(b == a + 1 for a, b in zip(ids, ids[1:]))
    assert any(p["count"] == hist for p in planted), "no planted rejection on a full window"
    accepted_before = np.cumsum([0] + [int(p["accepted"]) for p in pushes])
    assert any(accepted_before[p["push"]] >= hist + 2 for p in planted), "no planted rejection after the ring wrapped"
    # bookkeeping of the generator itself
    assert seq.count == min(hist, seq.accepted_total)
    assert all(0 <= p["slot"] <= hist for p in pushes)


def test_two_loop_references_agree_on_a_tiny_window():
    """two_loop64 against the closed form on one pair, and the fp32 torch-style recursion against it."""
    rng = np.random.default_rng(3)
    g, s = rng.standard_normal(50).astype(np.float32), rng.standard_normal(50).astype(np.float32)
    y = (2.0 * s + 0.1 * rng.standard_normal(50)).astype(np.float32)
    g64, s64, y64 = (v.astype(np.float64) for v in (g, s, y))
    ys, yy = s64 @ y64, y64 @ y64
    H, rho = ys / yy, 1.0 / ys
    # d = -(V^T H V + rho s s^T) g with V = I - rho y s^T
    q = g64 - rho * (s64 @ g64) * y64
    r = H * q
    r = r - rho * (y64 @ r) * s64 + rho * (s64 @ g64) * s64
    d = lr.two_loop64(g, [s], [y], H)
    np.testing.assert_allclose(d, -r, rtol=0, atol=1e-14 * np.abs(r).max())
    d32 = lr.two_loop32(g, [s], [y])
    assert np.abs(d32 - d).max() <= 1e-5 * np.abs(d).max()
    assert np.array_equal(lr.two_loop32(g, [], []), -g)
