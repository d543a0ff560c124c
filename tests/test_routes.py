"""The routing table of the extension terms, pinned: which terminal optim_chamfer / optim_markers reach -- the fused solve
(ChamferProblem / MarkerProblem), the frame-sharded solve or the closure composed from the operators -- or which refusal they
raise, over a grid of term combinations, execution switches, frame sharding, placements, contact labels and prior weights; and
what lockstep_supported answers for every configuration of that grid.  The terminals are replaced by recorders, so nothing is
solved and no kernel runs.  tests/routes_recorded.json holds the answers of the commit before the term table
(uuo_mocap_amd/terms.py) existed; every case must still give exactly its recorded answer, message texts included.

    python tests/test_routes.py [--device cuda] [--out FILE]

walks the grid on that device and writes its section of the record (the other sections are kept)."""
import contextlib
import copy
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "routes_recorded.json")
F, M, V = 6, 4, 6890

#: grid term -> (its execution switch or None, where its key goes: "losses" or the stage itself, the value that turns it on)
TERMS = {
    "robust_sigma": ("robust_fused", "stage", 0.05),
    "joint_accel": ("temporal_fused", "losses", 1.0),
    "foot_lock": ("temporal_fused", "losses", 1.0),
    "floor_penetration": ("floor_fused", "losses", 1.0),
    "floor_contact": ("floor_fused", "losses", 1.0),
    "self_penetration": ("capsule_fused", "losses", 1.0),
    "joint_limits": ("limit_fused", "losses", 1.0),
    "prior_confidence": ("prior_conf_fused", "stage", {"gap_weight": 0.3, "ramp": 2, "joint_weights": None}),
    "pose_accel": (None, "losses", 1.0),
}
TERMINALS = ("_optim_chamfer_general", "_optim_chamfer_frame_sharded", "ChamferProblem", "_optim_markers_general",
             "_optim_markers_frame_sharded", "MarkerProblem")
#: the stage's own axes: chamfer (soft_chamfer, surface_chamfer, yaw_lock), marker (placement, latent_offsets)
STAGE_AXES = {"chamfer": list(itertools.product((False, True), (False, True), (True, False))),
              "marker": list(itertools.product(("one_hot", "three", "four", "frame_table"), (False, True)))}
CONTACTS = ("absent", "zero", "two_frames")
PRIOR_WEIGHTS = ("absent", "ones", "with_zero")


class _Smpl:
    class device_model:
        V = V


class _Reached(Exception):
    pass


def _combos():
    """(terms, switched-off execution keys): no term, every term alone and every pair, each with the default execution block
    and with each involved term's own switch False"""
    names = list(TERMS)
    for terms in [()] + [(a,) for a in names] + list(itertools.combinations(names, 2)):
        switches = []
        for t in terms:
            if TERMS[t][0] is not None and TERMS[t][0] not in switches:
                switches.append(TERMS[t][0])
        for off in [None] + switches:
            yield terms, off


def _config(base, stage, terms, off, axes):
    cfg = copy.deepcopy(base)
    st = cfg["stages"][stage]
    for t in terms:
        _, where, value = TERMS[t]
        (st if where == "stage" else st["losses"])[t] = copy.deepcopy(value)
    if off is not None:
        cfg["execution"] = {off: False}
    if stage == "chamfer":
        soft, surface, yaw_lock = axes
        if soft:
            st["losses"]["soft_chamfer"] = 10.0
        if surface:
            st["losses"]["surface_chamfer"] = 10.0
            st["losses"]["full_chamfer"] = 0.0
            st["surface_distance"] = 0.0095
        st["yaw_lock"] = yaw_lock
    elif axes[1]:
        st["losses"]["latent_offsets"] = 1.0
    return cfg


def _tensors(device):
    z = lambda *s: torch.zeros(*s, device=device)
    placement = {"one_hot": z(M, V), "three": z(M, V), "four": z(M, V), "frame_table": None}
    placement["one_hot"][:, 0] = 1.0
    placement["three"][:, :3] = torch.tensor([0.5, 0.25, 0.25], device=device)
    placement["four"][:, :4] = 0.25
    two = z(F, 2)
    two[2:4, 0] = 1.0
    with_zero = torch.ones(F, 23, device=device)
    with_zero[1, 5] = 0.0
    return {"head": (z(F, M, 3), z(F, 23, 3, 3), z(F, 23, 3, 3), z(1, 10), z(1, 10), z(F, 1, 3, 3), z(F, 3)),
            "mask": z(F), "labels": torch.zeros(F, M, dtype=torch.long, device=device), "placement": placement,
            "frame_table": torch.zeros(F, M, dtype=torch.int32, device=device),
            "contacts": {"absent": None, "zero": z(F, 2), "two_frames": two},
            "prior_weights": {"absent": None, "ones": torch.ones(F, 23, device=device), "with_zero": with_zero}}


@contextlib.contextmanager
def _recorders(opt):
    """every terminal of the two stage solvers raises _Reached with its name and whether the `prior_weights` and `frame_assign`
    it was handed are None"""
    saved = {name: getattr(opt, name) for name in TERMINALS}

    def recorder(name, sig):
        def reached(*a, **k):
            got = sig.bind(*a, **k).arguments
            raise _Reached("-> %s prior_weights=%s frame_assign=%s" % (
                name, "None" if got.get("prior_weights") is None else "table",
                "None" if got.get("frame_assign") is None else "table"))
        return reached

    try:
        for name, fn in saved.items():
            setattr(opt, name, recorder(name, inspect.signature(fn)))
        yield
    finally:
        for name, fn in saved.items():
            setattr(opt, name, fn)


def _outcome(call):
    try:
        call()
    except _Reached as r:
        return str(r)
    except Exception as e:  # a refusal: its type and its full text
        return "%s: %s" % (type(e).__name__, e)
    return "returned without reaching a terminal"


def walk(device="cpu"):
    """Yields (case, outcome) over the whole grid, in a fixed order."""
    from uuo_mocap_amd import optimization as opt
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.config import packaged_config

    base = packaged_config("video_mocap")
    t = _tensors(torch.device(device))
    with _recorders(opt):
        for stage, sharded in itertools.product(("chamfer", "marker"), (False, True)):
            with (parallel.shard_frames(joint_with_one_rank=True) if sharded else contextlib.nullcontext()):
                for (terms, off), axes in itertools.product(_combos(), STAGE_AXES[stage]):
                    cfg = _config(base, stage, terms, off, axes)
                    for contacts, weights in itertools.product(CONTACTS, PRIOR_WEIGHTS):
                        kw = {"foot_contacts": t["contacts"][contacts], "prior_weights": t["prior_weights"][weights]}
                        if stage == "chamfer":
                            call = lambda: opt.optim_chamfer(*t["head"], t["mask"], t["labels"], None, cfg, **kw)
                        else:
                            if axes[0] == "frame_table":
                                kw["frame_assign"] = t["frame_table"]
                            call = lambda: opt.optim_markers(*t["head"], t["placement"][axes[0]], t["mask"], _Smpl, cfg, **kw)
                        case = "%s sharded=%d terms=%s off=%s axes=%s contacts=%s prior_weights=%s" % (
                            stage, sharded, "+".join(terms) or "-", off, "/".join(str(a) for a in axes), contacts, weights)
                        yield case, _outcome(call)


def walk_lockstep():
    """Yields (case, outcome) of lockstep_supported for every configuration of the grid."""
    from uuo_mocap_amd.config import packaged_config
    from uuo_mocap_amd.optimization import lockstep_supported

    base = packaged_config("video_mocap")
    for stage in ("chamfer", "marker"):
        axes_list = STAGE_AXES[stage] if stage == "chamfer" else [("one_hot", False), ("one_hot", True)]
        for (terms, off), axes in itertools.product(_combos(), axes_list):
            cfg = _config(base, stage, terms, off, axes)

            def call():
                raise _Reached("-> %s" % lockstep_supported(cfg, stage))

            yield "%s terms=%s off=%s axes=%s" % (stage, "+".join(terms) or "-", off, "/".join(str(a) for a in axes)), \
                _outcome(call)


def _encode(pairs, outcomes):
    """the outcomes of a walk as indices into `outcomes` (extended in place), in walk order"""
    out = []
    for _, o in pairs:
        if o not in outcomes:
            outcomes.append(o)
        out.append(outcomes.index(o))
    return out


def _check(section, pairs):
    with open(RECORD) as f:
        rec = json.load(f)
    want = rec[section]
    pairs = list(pairs)
    assert len(pairs) == len(want), "the grid has %d cases, the record %d" % (len(pairs), len(want))
    wrong = [(case, rec["outcomes"][w], got) for (case, got), w in zip(pairs, want) if rec["outcomes"][w] != got]
    assert not wrong, "%d of %d cases left their recorded route; the first:\n%s" % (
        len(wrong), len(pairs), "\n".join("%s\n  recorded: %s\n  now:      %s" % w for w in wrong[:10]))


def test_routes_on_the_host_match_the_record():
    _check("cpu", walk("cpu"))


def test_lockstep_supported_matches_the_record():
    _check("lockstep", walk_lockstep())


@pytest.mark.gpu
def test_routes_on_the_device_match_the_record():
    """the same walk with every tensor on the device: the fused soft-assignment closure and the fused surface / three-corner
    closures are in reach only there (`is_cuda`).  Small allocations only; nothing is launched."""
    _check("cuda", walk("cuda"))


if __name__ == "__main__":
    import argparse

    sys.path.insert(0, ROOT)
    ap = argparse.ArgumentParser(description="record the routing table (tests/routes_recorded.json)")
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    ap.add_argument("--out", default=RECORD)
    args = ap.parse_args()
    rec = {"outcomes": []}
    for path in (args.out, RECORD):
        if os.path.isfile(path):
            with open(path) as f:
                rec = json.load(f)
            break
    rec[args.device] = _encode(walk(args.device), rec["outcomes"])
    if args.device == "cpu":
        rec["lockstep"] = _encode(walk_lockstep(), rec["outcomes"])
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, indent=1 if k == "outcomes" else None, separators=(",", ":")))
                                   for k, v in rec.items()) + "\n}\n")
    print("%s: %d cases, %d distinct outcomes in all -> %s" % (args.device, len(rec[args.device]), len(rec["outcomes"]), args.out))
