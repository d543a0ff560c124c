"""The pruned nearest-vertex search (k_nn_cull) with its box table in global memory, LDS arrays sized by the launch and a
survivor list that is filled in batches: keys (distance bits << 32 | vertex) bit for bit against the CPU brute-force loop
(oracle/knn_cpu.c, first index on ties), and the survivor counts it reports against the same box test restated in numpy.

The kernel is reached through the debug library's search entry on the test's own clouds (the closure cannot place a duplicate
vertex or seed a previous assignment): the synthetic model's template at V = 6890 (431 units: a last super-box of 7 units, a
last unit of 10 vertices), three frames, and a cloud of V = 40 (3 units, less than one super-box).

One CPU-side check reads the built library's code object: five search blocks of the benchmark's shape fit into the LDS and
the registers that a k_skin3 block leaves on a CU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import p3d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 3
V_BODY, V_SMALL = 6890, 40
M_CASES = (1, 13, 14, 50, 64, 65)
f32 = np.float32

# what a k_skin3 block leaves of a CU (csrc/smpl_kernels.hip, SK3_LDS_PAD): LDS bytes, and VGPRs per lane beside its 191
LDS_CU, LDS_SKIN3, VGPR_FILE, VGPR_SKIN3 = 163840, 110592, 512, 191
BLOCKS_BESIDE_SKIN3 = 5


# ------------------------------------------------------------------------------------------------ CPU restatements
def _groups(Fr, M):
    """Marker groups of the launch (uuo_launch_nn_cull): (groups per frame, markers per group)."""
    G = (M + 63) // 64
    while G < 8 and Fr * G < 1024 and (M + G) // (G + 1) >= 8:
        G += 1
    return G, (M + G - 1) // G


def _boxes(verts):
    """Unit boxes as the skinning epilogue leaves them: exact fp32 min / max of each 16 vertices, the last unit padded with
    the last vertex.  [F][units][6]"""
    Fr, V, _ = verts.shape
    nu = (V + 15) // 16
    vp = np.concatenate([verts, np.repeat(verts[:, V - 1:V], nu * 16 - V, axis=1)], 1).reshape(Fr, nu, 16, 3)
    return np.ascontiguousarray(np.concatenate([vp.min(2), vp.max(2)], -1), dtype=f32)


def _sqdist(q, p):
    """((dx dx + dy dy) + dz dz) in fp32, every operation rounded on its own (the kernel's and the oracle's order)."""
    d = (q.astype(f32) - p.astype(f32)).astype(f32)
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def _lower_bounds(box, q):
    """The kernel's box bound of markers q [M][3] against boxes [U][6]: [M][U], fp32 operation by operation."""
    lo, hi = box[None, :, :3], box[None, :, 3:]
    d = np.maximum(np.maximum((lo - q[:, None, :]).astype(f32), (q[:, None, :] - hi).astype(f32)), f32(0))
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def _expected_stats(verts, box, markers, prev):
    """What the search reports per (frame, group): the number of (marker, unit) pairs whose box bound is <= the distance to the
    marker's previous vertex (out of range: vertex 0) -- or minus the number of all pairs where more than three quarters of
    the group's (marker, super-box) pairs pass (the enumerate path)."""
    Fr, V, _ = verts.shape
    M = markers.shape[1]
    nu = box.shape[1]
    nsup = (nu + 7) // 8
    G, mper = _groups(Fr, M)
    out = np.zeros((Fr, 8), np.int32)
    for f in range(Fr):
        p = np.where(prev[f] >= V, 0, prev[f])
        ub = _sqdist(markers[f], verts[f][p])
        lb = _lower_bounds(box[f], markers[f])
        pad = np.concatenate([box[f], np.repeat(box[f][-1:], nsup * 8 - nu, 0)]).reshape(nsup, 8, 6)
        sup = np.concatenate([pad[..., :3].min(1), pad[..., 3:].max(1)], -1)
        lb2 = _lower_bounds(sup, markers[f])
        for g in range(G):
            m = slice(g * mper, min(M, (g + 1) * mper))
            mg = m.stop - m.start
            found2 = int((lb2[m] <= ub[m, None]).sum())
            out[f, g] = -(nu * mg) if 4 * found2 > 3 * nsup * mg else int((lb[m] <= ub[m, None]).sum())
    return out


def _ref_keys(verts, markers):
    d, i = p3d_ref.knn1_loop(markers, verts)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)


def _keys_with(prev):
    """Input keys: the previous assignment in the low word; the search forms the distance itself (a stale one above it)."""
    return (np.uint64(0x3F800000) << np.uint64(32)) | prev.astype(np.uint64)


# ------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope="module")
def search():
    """search(verts, markers, keys_in) -> (keys, stats [F][8]): one launch of the pruned search on the debug library."""
    import torch

    from uuo_mocap_amd import _lib

    dbg = _lib.load_debug()
    fn = dbg.uuo_debug_nn_cull
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    dev = torch.device("cuda:0")

    def run(verts, markers, keys_in):
        Fr, V, _ = verts.shape
        M = markers.shape[1]
        dv, db, dm = (torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev) for a in (verts, _boxes(verts), markers))
        dk = torch.from_numpy(keys_in.astype(np.uint64).view(np.int64).copy()).to(dev)
        ds = torch.zeros((Fr, 8), dtype=torch.int32, device=dev)
        rc = fn(None, Fr, M, V, dm.data_ptr(), dv.data_ptr(), db.data_ptr(), dk.data_ptr(), ds.data_ptr())
        assert rc == 0, dbg.uuo_last_error()
        torch.cuda.synchronize()
        return dk.cpu().numpy().view(np.uint64), ds.cpu().numpy()

    return run


@pytest.fixture(scope="module")
def capacity():
    """Entries of the survivor list, from the library."""
    from uuo_mocap_amd import _lib

    out = (ctypes.c_int * 4)()
    assert _lib.load_debug().uuo_debug_nn_cull_geometry(F, 14, 431, out) == 0
    assert (out[0], out[1]) == _groups(F, 14) == (1, 14)
    return out[3]


@pytest.fixture(scope="module")
def body(tables):
    """Three frames of the template, each turned and moved a little."""
    vt = np.asarray(tables.v_template, dtype=np.float64)
    frames = []
    for f in range(F):
        a = 0.3 * f
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        frames.append(vt @ R.T + np.array([0.05 * f, 0.0, 0.1 * f]))
    verts = np.ascontiguousarray(np.stack(frames), dtype=f32)
    assert verts.shape == (F, V_BODY, 3)
    return verts


@pytest.fixture(scope="module")
def small():
    return np.ascontiguousarray(np.random.default_rng(11).uniform(0.0, 1.0, (F, V_SMALL, 3)), dtype=f32)


def _markers_near(verts, M, seed, off=0.03):
    """M markers per frame, each `off` metres (a standard deviation per axis) from a random vertex of its frame."""
    rng = np.random.default_rng(seed)
    vid = rng.integers(0, verts.shape[1], (verts.shape[0], M))
    base = np.take_along_axis(verts, vid[..., None], 1)
    return np.ascontiguousarray(base + off * rng.standard_normal(base.shape), dtype=f32)


def _check(search, verts, markers, keys_in, prev, tag):
    keys, stats = search(verts, markers, keys_in)
    want = _ref_keys(verts, markers)
    bad = np.argwhere(keys.reshape(want.shape) != want)
    assert len(bad) == 0, (tag, len(bad), bad[:5].tolist())
    exp = _expected_stats(verts, _boxes(verts), markers, prev)
    print("%s: survivors per (frame, group) %s" % (tag, stats.tolist()))
    assert np.array_equal(stats, exp), (tag, stats.tolist(), exp.tolist())
    return keys.reshape(want.shape), stats


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ("body", "small"))
@pytest.mark.parametrize("M", M_CASES)
def test_keys_bit_for_bit_first_and_second_call(search, body, small, cloud, M):
    """One group (M = 1, 13, 14), ragged last groups (50: 7 x 8 and 2; 65: 7 x 9 and 2), eight full groups (64): the first
    call (no previous keys), then markers moved by a few millimetres on the first call's assignment."""
    verts = body if cloud == "body" else small
    G, mper = _groups(F, M)
    assert {1: (1, 1), 13: (1, 13), 14: (1, 14), 50: (7, 8), 64: (8, 8), 65: (8, 9)}[M] == (G, mper)
    markers = _markers_near(verts, M, 100 + M)
    none = np.full((F, M), 0xFFFFFFFF, np.uint64)
    keys, _ = _check(search, verts, markers, np.full((F, M), ~np.uint64(0)), none, "%s M=%d first" % (cloud, M))
    moved = np.ascontiguousarray(markers + f32(0.003) * np.random.default_rng(M).standard_normal(markers.shape), dtype=f32)
    prev = keys & np.uint64(0xFFFFFFFF)
    _, stats = _check(search, verts, moved, keys, prev, "%s M=%d second" % (cloud, M))
    if cloud == "body":   # good bounds: every block prunes
        assert (stats[:, :G] > 0).all() and not stats[:, G:].any()


def _seeded(verts, markers, n_loose):
    """Previous assignments: the true nearest vertex (the tightest bound), but the FARTHEST vertex for the first n_loose
    markers of every frame -- every box passes for those."""
    d = ((markers[:, :, None, :].astype(np.float64) - verts[:, None, :, :]) ** 2).sum(-1)
    prev = d.argmin(-1).astype(np.uint64)
    prev[:, :n_loose] = d.argmax(-1)[:, :n_loose]
    return prev


@pytest.mark.gpu
@pytest.mark.parametrize("n_loose,lo,hi", [(3, 1.0, 2.0), (8, 3.0, 4.0)])
def test_list_is_drained_and_refilled(search, body, capacity, n_loose, lo, hi):
    """14 markers in one block, some with a far previous vertex: 3 of them list 3 x 431 pairs and a few (a little over the
    list's 1024 entries: two batches), 8 list 3448 and a few (more than three times: four batches; 60 % of the block's
    super-box pairs pass, short of the three quarters at which it would enumerate).  The count reported is
    positive -- the batches ran, not the enumerate path -- and the keys are the brute-force ones."""
    verts = body
    markers = _markers_near(verts, 14, 20)
    prev = _seeded(verts, markers, n_loose)
    _, stats = _check(search, verts, markers, _keys_with(prev), prev, "refill, %d loose" % n_loose)
    assert (stats[:, 0] > lo * capacity).all() and (stats[:, 0] < hi * capacity).all(), (stats.tolist(), capacity)


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ("body", "small"))
def test_all_loose_bounds_enumerate(search, body, small, cloud):
    verts = body if cloud == "body" else small
    markers = _markers_near(verts, 14, 23)
    prev = _seeded(verts, markers, 14)
    _, stats = _check(search, verts, markers, _keys_with(prev), prev, "all loose, " + cloud)
    assert (stats[:, 0] == -14 * ((verts.shape[1] + 15) // 16)).all(), stats.tolist()


@pytest.mark.gpu
def test_lower_index_wins_a_tie_across_batches(search, body, capacity):
    """Vertex 40 (unit 2, the first super-box) copied to vertex 6805 (unit 425, the last super-box), and vertex 6850 copied
    down to vertex 100; eight loose markers make the block run four batches, so the two units of a pair are tested batches
    apart.  Markers sit a tenth of a millimetre from the duplicated vertices and exactly on them, with the previous
    assignment far away, a neighbour, the higher copy and the lower one: the lower index wins every time."""
    verts = body.copy()
    verts[:, 6805] = verts[:, 40]
    verts[:, 100] = verts[:, 6850]
    markers = _markers_near(verts, 14, 21)
    for m, v in ((0, 40), (1, 40), (2, 100), (3, 100)):   # among the loose ones
        markers[:, m] = verts[:, v] + f32(1e-4)
    on_vertex = {8: (40, 6805), 9: (40, 40), 10: (40, 41), 11: (100, 6850), 12: (100, 100), 13: (100, 101)}
    for m, (v, p) in on_vertex.items():   # distance 0: the bound of the lower copy's unit (0) equals d_ub where p is a copy
        markers[:, m] = verts[:, v]
    prev = _seeded(verts, markers, 8)
    for m, (v, p) in on_vertex.items():
        prev[:, m] = p
    keys, stats = _check(search, verts, markers, _keys_with(prev), prev, "ties")
    assert (stats[:, 0] > 3 * capacity).all(), stats.tolist()
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (idx[:, [0, 1, 8, 9, 10]] == 40).all() and (idx[:, [2, 3, 11, 12, 13]] == 100).all(), idx.tolist()
    assert ((keys[:, 8:] >> np.uint64(32)) == 0).all()


@pytest.mark.gpu
def test_bound_equal_to_the_previous_distance_and_markers_on_box_faces(search, body):
    """Per frame, a = the vertex of largest x, copied to the higher vertex 6889 (another unit); the marker a + (0.5, 0, 0) with
    previous vertex 6889 has d_ub = (x + 0.5 - x)^2 = the bound of a's unit exactly (a is its max-x face, y and z inside), and
    the `<=` of the box test must keep that unit for a to win the tie.  Further markers lie exactly on a face of a unit's box
    (bound 0) and exactly on vertices, all in a block that takes the box test (13 markers, tight bounds)."""
    verts = body.copy()
    a = verts[:, :6880, 0].argmax(1)
    fr = np.arange(F)
    verts[:, 6889] = verts[fr, a]
    box = _boxes(verts)
    markers = _markers_near(verts, 13, 22)
    markers[:, 0] = verts[fr, a] + np.array([0.5, 0, 0], f32)
    for m, u in ((1, 0), (2, 215), (3, 430)):   # on the max-y face of unit u, at the middle of its x and z range
        markers[:, m, 0] = (box[:, u, 0] + box[:, u, 3]) / 2
        markers[:, m, 1] = box[:, u, 4]
        markers[:, m, 2] = (box[:, u, 2] + box[:, u, 5]) / 2
    for m, v in ((4, 0), (5, 3333), (6, 6888)):
        markers[:, m] = verts[:, v]
    prev = _seeded(verts, markers, 0)
    prev[:, 0], prev[:, 5] = 6889, 3000
    for f in range(F):
        lb = _lower_bounds(box[f], markers[f, :1])[0, a[f] // 16]
        assert lb == _sqdist(markers[f, 0], verts[f, 6889]) and lb > 0.2, (f, lb)
    keys, stats = _check(search, verts, markers, _keys_with(prev), prev, "equal bound")
    assert (stats[:, 0] > 0).all(), stats.tolist()
    assert ((keys[:, 0] & np.uint64(0xFFFFFFFF)) == a.astype(np.uint64)).all()
    assert ((keys[:, 4:7] >> np.uint64(32)) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ("body", "small"))
def test_previous_assignment_out_of_range(search, body, small, cloud):
    """Previous vertices V, 2^31 and 2^32 - 2 among valid ones: taken as vertex 0, the brute-force result."""
    verts = body if cloud == "body" else small
    V = verts.shape[1]
    markers = _markers_near(verts, 13, 24)
    prev = _seeded(verts, markers, 0)
    prev[:, 0], prev[:, 5], prev[:, 12] = V, 1 << 31, 0xFFFFFFFE
    _check(search, verts, markers, _keys_with(prev), prev, "previous out of range, " + cloud)


# ------------------------------------------------------------------------------------------------ residency (no GPU)
def test_five_blocks_fit_beside_a_skinning_block():
    """From the built library's code object: at the benchmark's shape (300 frames x 50 markers: 4 groups of 13, 431 units) a
    k_nn_cull block's static plus dynamic LDS fits five times into what a padded k_skin3 block leaves of a CU, and five of its
    waves fit beside a k_skin3 wave in a SIMD's register file."""
    from uuo_mocap_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    tools = [os.path.join(kernel_resources.LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(_lib.LIB_DEBUG_PATH) and all(os.path.isfile(t) for t in tools)):
        pytest.skip("needs the built libraries and the ROCm binutils")
    geo = (ctypes.c_int * 4)()
    assert _lib.load_debug().uuo_debug_nn_cull_geometry(300, 50, 431, geo) == 0
    assert (geo[0], geo[1]) == (4, 13)
    res = kernel_resources.resources(_lib.LIB_PATH)
    k = [v for name, v in res.items() if "k_nn_cull" in name and "k_nn_cull_b" not in name]
    assert len(k) == 1, sorted(res)
    lds = k[0][".group_segment_fixed_size"] + geo[2]
    print("k_nn_cull: %d B static + %d B dynamic LDS, %d VGPRs" % (k[0][".group_segment_fixed_size"], geo[2], k[0][".vgpr_count"]))
    assert BLOCKS_BESIDE_SKIN3 * lds <= LDS_CU - LDS_SKIN3, lds
    assert lds <= 10240, lds
    vgpr = 8 * ((k[0][".vgpr_count"] + 7) // 8)   # the allocation granule
    assert VGPR_SKIN3 + BLOCKS_BESIDE_SKIN3 * vgpr <= VGPR_FILE, k[0]
    assert k[0][".private_segment_fixed_size"] == 0
