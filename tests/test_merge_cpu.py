"""The merge's contract on its NumPy restatement alone (tests/merge_ref.py): the cases'
counts as conditions on the inputs, the properties the rules were chosen for, and what the method
reaches on two lounge submaps.  No device."""
import numpy as np
import pytest

from conftest import load_lounge, lounge_intrinsics
import merge_ref as M
from test_track_cpu import C1

F32 = np.float32
# mean, 95th percentile and maximum |dtsdf| * trunc in millimetres of the seeded 5 cm / 3 degree lounge
# join, measured from the restatement (4 cm voxels, truncation 20 cm).  The maximum sits at depth
# discontinuities, where five frames of one submap and ten of the whole map disagree about the surface
# by most of the band; its doubled bound is near the 400 mm the band allows and says little.  The
# mean and the percentile are the bounds that test the join away from those edges.
LOUNGE_MEASURED = (4.104, 14.14, 166.6)


@pytest.mark.parametrize("name", [k for k, v in M.CASES.items() if v[2]])
def test_case_counts(name):
    """outside / unseen / samples of each case are those of the CPU prototype of rules 1-3."""
    _, r = M.case_result(name)
    assert M.counts(r["code"]) == M.CASES[name][2]
    assert r["info"]["samples"] == M.CASES[name][2][2]


def test_cases_cover_every_code_and_degeneracy():
    codes = {k: 0 for k in (M.OUTSIDE, M.UNSEEN, M.SAMPLE)}
    ndeg = np.zeros(4, np.int64)
    for name in M.CASES:
        _, r = M.case_result(name)
        for k in codes:
            codes[k] += int((r["code"] == k).sum())
        ndeg += np.bincount(r["ndeg"][r["code"] == M.SAMPLE], minlength=4)
    assert min(codes.values()) >= 20
    assert ndeg.min() >= 20, ndeg
    # the cases the issue names by their degenerate axes
    for name, k in (("ident", 3), ("shift", 3), ("half", 2), ("turn", 1)):
        _, r = M.case_result(name)
        assert set(np.unique(r["ndeg"][r["code"] == M.SAMPLE])) == {k}, name
    _, r = M.case_result("big")
    assert (r["info"]["bricks_updated"], 12 * 9 * 8) == (360, 864)
    _, r = M.case_result("fine")
    assert int((np.abs(r["sample"]["rv"][r["code"] == M.SAMPLE]) > 1).sum()) >= 20  # (rho = 2 clamps)


@pytest.mark.parametrize("name", ["ident", "shift"])
def test_whole_voxel_translation_copies_bit_for_bit(name):
    """Into an empty destination, every sampled voxel is the source voxel it lands on: tsdf, weight
    and colour, the high faces included (the degenerate-axis rule)."""
    dst, T, _ = M.CASES[name]
    _, r = M.case_result(name)
    s_t, s_w, s_c = M.source_state()
    k = np.rint(-T[:3, 3] / dst.vs).astype(int)  # destination index + k = source index
    m = r["code"] == M.SAMPLE
    idx = np.nonzero(m)
    src = tuple(idx[a] + k[a] for a in range(3))
    for got, want in ((r["tsdf"], s_t), (r["weight"], s_w), (r["color"], s_c)):
        assert got[idx].tobytes() == want[src].tobytes()
    # and every observed source voxel that lands inside the destination was sampled
    seen = np.zeros(dst.dims, bool)
    lo = [max(0, -k[a]) for a in range(3)]
    hi = [min(dst.dims[a], M.SRC.dims[a] - k[a]) for a in range(3)]
    sl_d = tuple(slice(lo[a], hi[a]) for a in range(3))
    sl_s = tuple(slice(lo[a] + k[a], hi[a] + k[a]) for a in range(3))
    seen[sl_d] = s_w[sl_s] > 0
    assert np.array_equal(seen, m)
    for a, v in ((r["tsdf"], 1.0), (r["weight"], 0.0), (r["color"], 0.0)):
        assert (a[~m] == F32(v)).all()


@pytest.mark.parametrize("name", ["rot", "big", "fine"])
def test_prefilled_destination(name):
    """Unsampled voxels keep their bytes, canonical inputs give canonical outputs, and the sampled
    ones move: weights grow by the sample's."""
    (t0, w0, c0, mask0), r = M.case_result(name, filled=True)
    m = r["code"] == M.SAMPLE
    assert m.sum() == M.CASES[name][2][2] and (mask0 & m).sum() >= 20 and (mask0 & ~m).sum() >= 20
    for got, was in ((r["tsdf"], t0), (r["weight"], w0), (r["color"], c0)):
        assert got[~m].tobytes() == was[~m].tobytes()
    assert np.array_equal(r["mask"], mask0 | m)
    w, c = r["weight"], r["color"]
    assert (w == np.trunc(w)).all() and (w >= 0).all()
    assert (c == np.trunc(c)).all() and (c >= 0).all() and (c < 2 ** 24).all()
    assert np.array_equal(w[m], w0[m] + r["sample"]["w"][m]) and (r["sample"]["w"][m] >= 1).all()
    assert np.abs(r["tsdf"]).max() <= 1.0


def test_two_merges_add_twice_the_weight():
    dst, T, _ = M.CASES["rot"]
    (t0, w0, c0, _), r1 = M.case_result("rot", filled=True)
    r2 = M.merge(dst, r1["tsdf"], r1["weight"], r1["color"], M.SRC, *M.source_state(), T)
    m = r1["code"] == M.SAMPLE
    assert np.array_equal(r2["code"], r1["code"])
    assert np.array_equal(r2["weight"][m], w0[m] + 2 * r1["sample"]["w"][m])
    assert r2["weight"][~m].tobytes() == w0[~m].tobytes()


def test_transform_rule():
    assert M.check_transform(np.eye(4)) and M.check_transform(M.E)
    bad = [M.E.copy() for _ in range(5)]
    bad[0][:3, :3] *= 1.0 + 1e-5
    bad[1][:3, 0] *= -1.0
    bad[2][3, 0] = 1e-3
    bad[3][0, 3] = np.inf
    bad[4][1, 1] = np.nan
    assert not any(M.check_transform(b) for b in bad)


@pytest.fixture(scope="module")
def lounge_identity():
    return M.lounge_maps(np.eye(4), C1, load_lounge, lounge_intrinsics)


def test_lounge_submaps_identity(lounge_identity):
    """Frames 0-4 and 5-9 fused apart in one lattice and merged with the identity are the ten frames
    fused together: the weights exactly, the tsdf to the rounding of two weighted means."""
    geo, A, B, C = lounge_identity
    r = M.lounge_compare(geo, A, B, C, np.eye(4))
    print(r)
    assert r["n"] >= 1000
    assert r["weights_equal"]
    assert r["max_dt"] <= 1e-6


def test_lounge_submaps_moved():
    """The second submap lives in a world moved by a seeded 5 cm / 3 degree motion and is merged back
    under it: the join against the ten-frame map, within twice the measured figures."""
    G = M.rigid(M.LOUNGE_G_SEED, 0.05, 3.0)
    geo, A, B, C = M.lounge_maps(G, C1, load_lounge, lounge_intrinsics)
    r = M.lounge_compare(geo, A, B, C, G)
    print(r)
    assert r["n"] >= 1000
    assert r["mean_mm"] <= 2 * LOUNGE_MEASURED[0]
    assert r["p95_mm"] <= 2 * LOUNGE_MEASURED[1]
    assert r["max_mm"] <= 2 * LOUNGE_MEASURED[2]
