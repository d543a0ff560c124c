"""The general backward kernels on their phased LDS layout (csrc/closure.hip, BwdLdsPhased: the reduction's and the tail's arrays
take the bytes the item loop's leave; the pose features re-read from LDS inside the loop) against the same instantiations on one
array per name with the features in registers (the debug library's BWD_WIDE forms, UUO_BWD_WIDE_LDS=1): loss and the whole
gradient bit for bit, for the chamfer and the marker closure.

Marker counts against the block's 16 item slots: 1 (fewer items than slots), 15 (one short of a round), 16 (exactly one round), 17
(a ragged second round), 50 (the benchmark's four rounds), 65 (a fifth round); three frames; the start point and two perturbed
points each.  One shape with the joint-acceleration term on (video_mocap_smooth, F = 5, M = 17) covers the temporal instantiations,
whose window adds 2 080 B beside the overlay.

One CPU-side check reads the built product library's code object: two blocks of k_bwd_sparse (and of its lock-step batch twin) fit
into the LDS and the registers that a k_skin3 block leaves on a CU, without scratch."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_CASES = (1, 15, 16, 17, 50, 65)

# what a k_skin3 block leaves of a CU (csrc/smpl_kernels.hip, SK3_LDS_PAD): LDS bytes, and VGPRs per lane beside its 191
LDS_CU, LDS_SKIN3, VGPR_FILE, VGPR_SKIN3 = 163840, 110592, 512, 191
LDS_BWD_MAX = 25600  # fits twice into the 53 248 B left, up to an allocation granule of 1 280 B on both kernels


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def smpl(tables, dev):
    from uuo_mocap_amd.smpl import SmplInference

    return SmplInference(dev, tables=tables)


def _problem(smpl, dev, stage, config, F, M):
    """(problem, start point) of a synthetic sequence, as the suite builds them everywhere."""
    import torch

    from uuo_mocap_amd.config import packaged_config
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem
    from uuo_mocap_amd.synthetic import make_sequence

    seq = make_sequence(smpl.tables, seed=40 + M, num_frames=F, num_markers=M)
    cfg = packaged_config(config)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).to(dev)
    root = seq.img_smpl.root_orient.to(dev)
    trans0 = torch.median(markers, dim=1)[0]
    if stage == "chamfer":
        prob = ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg)
        x0 = prob.pack(trans0, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose)
    else:
        prob = MarkerProblem(smpl, markers, o_pose, o_betas, torch.from_numpy(seq.gt["marker_vids"]).to(dev), cfg)
        x0 = prob.pack(o_pose, o_betas, root, trans0)
    prob._need_workspace()
    return prob, x0


def _identical_on_both_layouts(prob, x0, dev, tag):
    import torch

    from uuo_mocap_amd import _lib
    from uuo_mocap_amd.engine import _ptr, current_stream

    dbg = _lib.load_debug()

    def evaluate(x, wide):
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        grad = torch.empty((prob.n,), dtype=torch.float32, device=dev)
        os.environ["UUO_BWD_WIDE_LDS"] = "1" if wide else "0"
        try:
            with torch.cuda.device(dev):
                prob._arm()
                rc = dbg.uuo_closure_eval(prob.fit, current_stream(dev), ctypes.byref(prob.problem), _ptr(x), _ptr(loss), _ptr(grad),
                                          None)
        finally:
            os.environ.pop("UUO_BWD_WIDE_LDS", None)
        assert rc == 0, dbg.uuo_last_error()
        torch.cuda.synchronize()
        return loss, grad

    gen = torch.Generator(device="cpu").manual_seed(7)
    points = [x0] + [(x0 + 0.01 * torch.randn(prob.n, generator=gen).to(dev)).contiguous() for _ in range(2)]
    for i, x in enumerate(points):
        lp, gp = evaluate(x, False)
        lw, gw = evaluate(x, True)
        assert torch.isfinite(lp).all() and torch.isfinite(gp).all() and float(gp.abs().max()) > 0, (tag, i)
        assert torch.equal(lp, lw) and torch.equal(gp, gw), (tag, i, float(lp), float(lw), float((gp - gw).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("M", M_CASES)
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_phased_lds_is_bit_identical_to_one_array_per_name(smpl, dev, stage, M):
    prob, x0 = _problem(smpl, dev, stage, "video_mocap", 3, M)
    _identical_on_both_layouts(prob, x0, dev, "%s M=%d" % (stage, M))


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["chamfer", "marker"])
def test_phased_lds_is_bit_identical_with_the_joint_acceleration_window(smpl, dev, stage):
    prob, x0 = _problem(smpl, dev, stage, "video_mocap_smooth", 5, 17)
    assert prob.joint_accel > 0
    _identical_on_both_layouts(prob, x0, dev, "%s smooth" % stage)


# ------------------------------------------------------------------------------------------------ residency (no GPU)
def test_two_blocks_fit_beside_a_skinning_block():
    """From the built product library's code object: k_bwd_sparse and its batch twin k_bwd_sparse_b hold at most 25 600 B of LDS
    and so few VGPRs (rounded up to the allocation granule of 8) that two of their waves fit beside a k_skin3 wave in a SIMD's
    register file, and use no scratch."""
    from uuo_mocap_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    tools = [os.path.join(kernel_resources.LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not (os.path.isfile(_lib.LIB_PATH) and all(os.path.isfile(t) for t in tools)):
        pytest.skip("needs the built library and the ROCm binutils")
    res = kernel_resources.resources(_lib.LIB_PATH)
    for entry in ("_Z12k_bwd_sparse7BwdArgs", "_Z14k_bwd_sparse_bPK7BwdArgs"):
        assert entry in res, sorted(k for k in res if "k_bwd_sparse" in k)
        k = res[entry]
        print("%s: %d B LDS, %d VGPRs, %d B scratch" % (entry, k[".group_segment_fixed_size"], k[".vgpr_count"],
                                                        k[".private_segment_fixed_size"]))
        assert k[".group_segment_fixed_size"] <= LDS_BWD_MAX, k
        assert 2 * LDS_BWD_MAX <= LDS_CU - LDS_SKIN3
        vgpr = 8 * ((k[".vgpr_count"] + 7) // 8)   # the allocation granule
        assert VGPR_SKIN3 + 2 * vgpr <= VGPR_FILE, k
        assert k[".private_segment_fixed_size"] == 0, k
