"""What the closures refuse about a workspace's side terms (csrc/closure.hip: side_term_rows, side_terms_check): the part stage,
the soft-assignment data term and lock-step recording, term by term, with the texts validate_problem carried before the table
existed (the joint-acceleration and foot-lock terms' lock-step texts are the evaluation's of that time, extended by the
parenthetical of the others).  Host code only: the debug library loads without a device (uuo_debug_term_refusal)."""
import pytest

from uuo_mocap_amd import _lib

NONE, PART, SOFT_CHAMFER, SOFT_PART, LOCKSTEP = range(5)
OFF, ALL = -1, -2

# (part stage, soft-assignment data term, lock-step recording) per term, in the table's order
EXPECTED = [
    ("closure: the joint-acceleration term (uuo_fit_set_joint_accel, extension) is not built for the part stage",
     "closure: the joint-acceleration term (uuo_fit_set_joint_accel, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the joint-acceleration term (uuo_fit_set_joint_accel, extension)"),
    ("closure: the foot-lock term (uuo_fit_set_foot_lock, extension) is not built for the part stage",
     "closure: the foot-lock term (uuo_fit_set_foot_lock, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the foot-lock term (uuo_fit_set_foot_lock, extension)"),
    ("closure: the floor-contact term (uuo_fit_set_floor, extension) is not built for the part stage",
     "closure: the floor-contact term (uuo_fit_set_floor, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the floor-contact term (uuo_fit_set_floor, extension)"),
    ("closure: the self-penetration term (uuo_fit_set_capsules, extension) is not built for the part stage",
     "closure: the self-penetration term (uuo_fit_set_capsules, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the self-penetration term (uuo_fit_set_capsules, extension)"),
    ("closure: the key-point reprojection term (uuo_fit_set_keypoints2d, extension) is not built for the part stage",
     "closure: the key-point reprojection term (uuo_fit_set_keypoints2d, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the key-point reprojection term (uuo_fit_set_keypoints2d, extension)"),
    ("closure: the joint-angle limit term (uuo_fit_set_joint_limits, extension) is not built for the part stage",
     "closure: the joint-angle limit term (uuo_fit_set_joint_limits, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the joint-angle limit term (uuo_fit_set_joint_limits, extension)"),
    ("closure: the pose-acceleration term (uuo_fit_set_pose_accel, extension) is not built for the part stage",
     "closure: the pose-acceleration term (uuo_fit_set_pose_accel, extension) is not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the pose-acceleration term (uuo_fit_set_pose_accel, extension)"),
    ("closure: the pose prior's weights (uuo_fit_set_prior_weights, extension) are not built for the part stage",
     "closure: the pose prior's weights (uuo_fit_set_prior_weights, extension) are not built for the soft-assignment data term (w_soft)",
     "closure: lock-step batches do not carry the pose prior's weights (uuo_fit_set_prior_weights, extension)"),
]
# the lock-step texts of the two oldest terms extend what the evaluation said before
OLD_EVALUATION_TEXTS = {0: "closure: lock-step batches do not carry the joint-acceleration term",
                        1: "closure: lock-step batches do not carry the foot-lock term"}


def _refusal(dbg, term, situation):
    rc = dbg.uuo_debug_term_refusal(term, situation)
    return rc, (dbg.uuo_last_error().decode() if rc else "")


@pytest.mark.parametrize("term", range(len(EXPECTED)))
def test_each_term_is_refused_with_the_text_it_always_had(term):
    dbg = _lib.load_debug()
    part, soft, lockstep = EXPECTED[term]
    assert _refusal(dbg, term, NONE) == (0, "")
    assert _refusal(dbg, term, PART) == (-22, part)
    assert _refusal(dbg, term, SOFT_CHAMFER) == (-22, soft)
    assert _refusal(dbg, term, SOFT_PART) == (-22, part)      # the part stage is looked at first, as before
    assert _refusal(dbg, term, LOCKSTEP) == (-22, lockstep)
    if term in OLD_EVALUATION_TEXTS:
        assert lockstep.startswith(OLD_EVALUATION_TEXTS[term])


def test_nothing_set_nothing_refused_and_everything_set_passes_where_it_is_built():
    dbg = _lib.load_debug()
    for situation in (NONE, PART, SOFT_CHAMFER, SOFT_PART, LOCKSTEP):
        assert _refusal(dbg, OFF, situation) == (0, "")
    assert _refusal(dbg, ALL, NONE) == (0, "")
    # with every term set the first row answers
    assert _refusal(dbg, ALL, PART) == (-22, EXPECTED[0][0])
    assert _refusal(dbg, ALL, LOCKSTEP) == (-22, EXPECTED[0][2])
    # one past the table
    rc, text = _refusal(dbg, len(EXPECTED), NONE)
    assert rc == -22 and "no such term" in text
