"""The backward-kernel selector of csrc/closure.hip (bwd_select: facts of a launch -> one row of the kernel table, by exact match of
the flag word) against a restatement of the `if` ladders it replaced, over every combination of the facts.  Host code only: the
debug library loads without a device (uuo_debug_bwd_select)."""
import ctypes
import itertools

from uuo_mocap_amd import _lib

CHAMFER, MARKER, PART, UPSTREAM = _lib.UUO_STAGE_CHAMFER, _lib.UUO_STAGE_MARKER, _lib.UUO_STAGE_PART, 3
ROOTS = (_lib.UUO_STAGE_ROOT, _lib.UUO_STAGE_ROOT_SHARED)
FACTS = ("stage", "part_cached", "one_wave", "three_corner", "surface", "soft_chamfer", "robust", "temporal", "offs", "fassign",
         "floor")
REFUSED, UNREACHABLE = "refused", "unreachable"


def _select(dbg, facts):
    arr = (ctypes.c_int * 11)(*[int(facts[f]) for f in FACTS])
    name, flags = ctypes.create_string_buffer(64), ctypes.c_uint(0)
    rc = dbg.uuo_debug_bwd_select(arr, 0, name, ctypes.byref(flags))
    return (name.value.decode(), flags.value) if rc > 0 else (REFUSED, dbg.uuo_last_error().decode())


def _table(dbg):
    name, flags = ctypes.create_string_buffer(64), ctypes.c_uint(0)
    n = dbg.uuo_debug_bwd_select(None, 0, name, ctypes.byref(flags))
    rows = []
    for i in range(n):
        assert dbg.uuo_debug_bwd_select(None, i, name, ctypes.byref(flags)) == n
        rows.append((name.value.decode(), flags.value))
    assert dbg.uuo_debug_bwd_select(None, n, name, ctypes.byref(flags)) == -22
    return rows


def _ladders(stage, part_cached, one_wave, three_corner, surface, soft_chamfer, robust, temporal, offs, fassign, floor):
    """What uuo_closure_eval_impl (and uuo_smpl_backward, stage 3) launched before the selector existed: the kernel's name,
    REFUSED where an earlier UUO_REQUIRE turned the combination away, UNREACHABLE where no problem produces it."""
    r = "_r" if robust else ""
    if stage == UPSTREAM:  # uuo_smpl_backward: the dense route or the sparse gather, nothing else
        if part_cached or three_corner or surface or robust or temporal or offs or fassign or floor:
            return UNREACHABLE
        return "k_bwd_dense" if soft_chamfer else "k_bwd_sparse"
    if stage in ROOTS:  # the part stage's kernel on all vertices, launched by hand before the selector named it; nothing else
        if part_cached or three_corner or surface or soft_chamfer or robust or temporal or offs or fassign or floor:
            return UNREACHABLE  # (validate_problem and side_terms_check turn every one of them away)
        return "k_bwd_root1" if one_wave else "k_bwd_root"
    # facts that are functions of one another: the cached pose blend is the part stage's, the three-corner placement and the
    # latent offsets are the marker stage's, the soft chamfer closure is the chamfer stage's, the floor term is a temporal term
    if (part_cached and stage != PART) or (three_corner and stage != MARKER) or (offs and stage != MARKER) or \
            (soft_chamfer and stage != CHAMFER) or (floor and not temporal):
        return UNREACHABLE
    # refused before any ladder: the per-frame vertex table outside the marker stage's plain one-hot closure, or with the floor term
    if fassign and not (stage == MARKER and not three_corner and not offs):
        return REFUSED
    if floor and fassign:
        return REFUSED
    if part_cached:
        return ("k_bwd_part1" if one_wave else "k_bwd_part") + r
    if three_corner:
        if floor:
            return "k_bwd_items_t_o_fl" if offs else "k_bwd_items_t_fl"
        if offs:
            return "k_bwd_items_t_o" if temporal else "k_bwd_items_o"
        return "k_bwd_items_t" if temporal else "k_bwd_items"
    if surface:
        if not (stage == CHAMFER and not soft_chamfer):  # refused at the head of the surface branch
            return REFUSED
        if floor:
            return "k_bwd_items_t_f_fl"
        return "k_bwd_items_t_f" if temporal else "k_bwd_items_f"
    if soft_chamfer:
        return "k_bwd_dense"
    if offs:
        if temporal:
            return "k_bwd_sparse%s_t_o%s" % (r, "_fl" if floor else "")
        return "k_bwd_sparse%s_o" % r
    if temporal:
        if floor:
            return "k_bwd_sparse%s_t_fl" % r
        if fassign:
            return "k_bwd_sparse%s_t_f" % r
        return "k_bwd_sparse%s_t" % r
    if fassign:
        return "k_bwd_sparse%s_f" % r
    return "k_bwd_sparse" + r


def test_selector_is_the_ladders_it_replaced():
    dbg = _lib.load_debug()
    rows = _table(dbg)
    names = {n for n, _ in rows}
    reached = set()
    for stage in (CHAMFER, MARKER, PART, UPSTREAM) + ROOTS:
        for bits in itertools.product((False, True), repeat=10):
            facts = dict(zip(FACTS, (stage,) + bits))
            want = _ladders(**facts)
            if want == UNREACHABLE:
                if stage in ROOTS:  # no problem produces it, and the selector does not lean on that
                    got, detail = _select(dbg, facts)
                    assert got == REFUSED and "no backward kernel" in detail and "stage %d" % stage in detail, (facts, got, detail)
                continue
            got, detail = _select(dbg, facts)
            assert got == want, (facts, got, detail)
            if want == REFUSED:
                assert "no backward kernel" in detail and "stage %d" % stage in detail, detail
            else:
                assert want in names
                reached.add(want)
    assert reached == names, names - reached                      # no row that nothing selects
    assert len({fl for _, fl in rows}) == len(rows) == len(names)  # no two rows behind one flag word, no name twice
