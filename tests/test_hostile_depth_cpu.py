"""The hostile f64 depth frames of tests/hostile_depth.py on the CPU alone: the oracle and the NumPy port
against the fixture the reference itself produced (tools/gen_golden.py, "hostile"), the conditions
the placement must meet for the device tests to mean something, and what the three tracking
restatements say about a pixel without a usable depth."""
import os

import numpy as np
import pytest

from conftest import GOLD
import hostile_depth as H
import icp_color_ref as C
import icp_ref as I
import oracle as O
import raycast_ref as R
import sdf_ref as S
import track_edge_cases as E


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "hostile_depth.npz"))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("size", list(H.SIZES))
def test_fixture_holds_the_shared_inputs(gold, size):
    """The frames the reference integrated are the ones hostile_depth.py builds, NaN payloads and
    signed zeros included."""
    names, depth, rgb, poses, ow = H.sequence(size)
    assert list(gold[size + "_names"]) == names and list(gold["class_names"]) == list(H.CLASSES)
    assert np.array_equal(bits(gold["class_values"]), bits(H.VALUES))
    assert np.array_equal(bits(gold[size + "_depth"]), bits(depth))
    assert np.array_equal(gold[size + "_rgb"][gold[size + "_rgb_index"]], rgb)
    assert np.array_equal(gold[size + "_poses"], poses) and np.array_equal(gold[size + "_obs_weight"], ow)
    assert np.array_equal(gold["K"], H.K) and np.array_equal(gold["bounds"], np.array(H.BOUNDS))
    assert depth.shape[1:] == H.SIZES[size] and (depth.shape[2] % 4 == 0) == (size == "vec")
    assert os.path.getsize(os.path.join(GOLD, "hostile_depth.npz")) < 640 * 1024


def _replay(gold, size, step):
    """step(f) integrates frame f and returns (update count, tsdf, weight, colour); each frame's state
    must equal the fixture's bit for bit, untouched voxels included."""
    n_vox = int(np.prod(H.DIMS))
    t, w, c = np.ones(n_vox, np.float32), np.zeros(n_vox, np.float32), np.zeros(n_vox, np.float32)
    for f in range(len(gold[size + "_names"])):
        p = "%s_f%d_" % (size, f)
        idx = np.flatnonzero(np.unpackbits(gold[p + "mask"])[:n_vox])
        t[idx], w[idx], c[idx] = gold[p + "tsdf"], gold[p + "weight"], gold[p + "color"]
        n, T, W, Cc = step(f)
        assert n == int(gold[p + "nupd"]) == len(idx), f
        assert np.array_equal(bits(T.reshape(-1)), bits(t)), f
        assert np.array_equal(bits(W.reshape(-1)), bits(w)) and np.array_equal(bits(Cc.reshape(-1)), bits(c)), f
    assert not (np.isnan(t).any() or np.isnan(w).any() or np.isnan(c).any())


@pytest.mark.parametrize("port", ["oracle", "numpy_port"])
@pytest.mark.parametrize("size", list(H.SIZES))
def test_oracle_and_numpy_port_match_the_reference_bit_for_bit(gold, size, port):
    _, depth, rgb, poses, ow = H.sequence(size)
    vol = O.OracleTSDFVolume(np.array(H.BOUNDS), H.VS)
    coords = O.vox_coords_for(vol._vol_dim)

    def step(f):
        with np.errstate(all="ignore"):
            n = (vol.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f])) if port == "oracle" else
                 O.numpy_port_integrate(vol, coords, rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f])))
        return n, vol._tsdf_vol_cpu, vol._weight_vol_cpu, vol._color_vol_cpu

    _replay(gold, size, step)


@pytest.mark.parametrize("size", list(H.SIZES))
def test_hash_oracle_matches_the_reference_hash_path(gold, size):
    """HashTable.integrate (f64 Voxel state, obs_weight ignored) over the same frames: the final
    entries and the entry count after every frame."""
    _, depth, rgb, poses, ow = H.sequence(size)
    hv = O.OracleHashVolume(np.array(H.BOUNDS), H.VS)
    for f in range(len(depth)):
        hv.integrate(rgb[f], depth[f], H.K, poses[f], obs_weight=float(ow[f]))
        assert len(hv.entries()[0]) == int(gold[size + "_hash_entries"][f]), f
    idx, sdf, w, c = hv.entries()
    n_vox = int(np.prod(H.DIMS))
    assert np.array_equal(idx, np.flatnonzero(np.unpackbits(gold[size + "_hash_mask"])[:n_vox]))
    assert np.array_equal(bits(sdf), bits(gold[size + "_hash_sdf"]))
    assert np.array_equal(w, gold[size + "_hash_weight"]) and np.array_equal(c, gold[size + "_hash_color"])
    assert not np.isnan(sdf).any()
    # the dense path over the same frames with weight 1 observes the same voxels
    dense, _ = H.oracle_run(size, obs_weight=1.0)
    assert np.array_equal(idx, np.flatnonzero(dense._weight_vol_cpu.reshape(-1) > 0))


@pytest.mark.parametrize("size", list(H.SIZES))
def test_coverage_conditions_hold_on_the_oracle(size):
    """Alone in its region of an otherwise zero frame: NaN, -inf, negatives and -0.0 change nothing;
    the tiny depths change the >= 10 voxels with 0 < z <= trunc (the same ones whether or not the
    depth survives a conversion to f32); +inf, the huge and the far depths carve >= 1000; no NaN
    reaches the state.  And the class region holds a whole prep tile with nothing else in it."""
    counts = H.assert_coverage(size)
    print(size, counts)
    assert len({counts[k] for k, (_, g) in H.CLASSES.items() if g == "tiny"}) == 1
    assert len({counts[k] for k, (_, g) in H.CLASSES.items() if g in ("carve", "far")}) == 1
    (r, c), (tr, tc) = H.region(size), H.whole_tile(size)
    assert r.start <= tr.start and tr.stop <= r.stop and c.start <= tc.start and tc.stop <= c.stop
    assert tr.start % 64 == 0 and tc.start % 64 == 0 and tr.stop - tr.start == 64 == tc.stop - tc.start
    assert tr.stop <= H.SIZES[size][0] and tc.stop <= H.SIZES[size][1]
    for name, (v, _) in H.CLASSES.items():
        tile = H.class_frame(size, name)[tr, tc]
        assert np.array_equal(bits(tile), bits(np.full(tile.shape, v))), name
    # the tiny classes' voxels lie in bricks that no other depth of their frame reaches a cull for:
    # the tile's pyramid maximum is the tiny depth alone
    vol, n = H.oracle_run(size)
    names = H.sequence(size)[0]
    assert n[names.index("all_nan")] == 0 and n[names.index("all_zero")] == 0
    assert all(n[names.index(k)] > 0 for k in H.CLASSES)  # (the background outside the region)
    assert not np.isnan(vol._tsdf_vol_cpu).any()


def test_scatter_frame_puts_every_class_at_every_block_position():
    for size, (Hh, W) in H.SIZES.items():
        d, bg = H.scatter_frame(size), H.background(size)
        y, x = np.nonzero(bits(d) != bits(bg))
        seen = set()
        for yy, xx in zip(y, x):
            k = int(np.flatnonzero(bits(H.VALUES) == bits(d[yy:yy + 1, xx])[0])[0])
            seen.add((k, (yy % 2) * 4 + xx % 4))
        assert len(seen) == 8 * len(H.VALUES), (size, len(seen))
        blocks = {(yy // 2, xx // 4) for yy, xx in zip(y, x)}
        assert len(blocks) == len(y)  # one hostile pixel per block: its neighbours in every fmaxf are valid


def test_frustum_cases_show_what_the_contract_speaks_of():
    """On the oracle alone: the finite frames have finite maxima and coordinates; of the contract
    frames the +inf one (seen through the rotation without a zero row entry) has NaN and infinite
    coordinates, the 1.7e308 one overflows to infinite ones, the bounds fold infinities and hold no
    NaN, and a frame of NaNs has max depth 0.0 and the camera centre as its frustum."""
    Hh, W = H.SIZES["vec"]
    finite, contract = H.frustum_frames("vec")
    md = np.array([O.frame_max_depth(f) for f in finite.values()])
    poses = H.frustum_poses(len(md))
    assert np.isfinite(md).all() and all(np.isfinite(O.view_frustum(m, Hh, W, H.K, p)).all() for m, p in zip(md, poses))
    assert np.array_equal(md, [np.fmax.reduce(f, axis=None) for f in finite.values()])
    # for finite maxima the rule is the demo's np.minimum / np.maximum
    ref = np.zeros((3, 2))
    for m, p in zip(md, poses):
        v = O.view_frustum(m, Hh, W, H.K, p)
        ref[:, 0], ref[:, 1] = np.minimum(ref[:, 0], v.min(axis=1)), np.maximum(ref[:, 1], v.max(axis=1))
    assert np.array_equal(bits(O.frustum_bounds(md, Hh, W, H.K, poses)), bits(ref))
    names = list(contract)
    md = [O.frame_max_depth(f) for f in contract.values()]
    assert names == ["pos_inf", "scatter", "huge_1.7e308", "all_nan", "all_nan_neg"] and md == [np.inf, np.inf, 1.7e308, 0.0, 0.0]
    poses = H.frustum_poses(len(md))
    pts = [O.view_frustum(m, Hh, W, H.K, p) for m, p in zip(md, poses)]
    assert np.isnan(pts[0]).any() and np.isinf(pts[0]).any() and np.isinf(pts[2]).any()
    b = O.frustum_bounds(md, Hh, W, H.K, poses)
    assert np.isinf(b).any() and not np.isnan(b).any()
    for f in (3, 4):
        assert np.array_equal(pts[f], np.repeat(poses[f][:3, 3:4], 5, axis=1))
    assert not np.isnan(O.frustum_bounds([np.inf], Hh, W, H.K, [np.eye(4)])).any()  # (every far point NaN: 0 * inf)


# ---- tracking restatements --------------------------------------------------------------------------
def test_the_tracking_rule_on_the_class_values():
    """f32(d) > 0 and finite: 1e-40 (an f32 subnormal), 65.535, 65.536 and 70 are depths; everything
    else in the table is none -- 5e-324 and 1e-46 round to zero, 3.5e38 and beyond to infinity."""
    bad = dict(zip(H.CLASSES, H.track_hostile(H.VALUES)))
    assert [k for k, v in bad.items() if not v] == ["tiny_1e-40", "d_65.535", "d_65.536", "d_70"]


@pytest.fixture(scope="module")
def corner_maps():
    t, w, c = I.corner_state()
    return R.raycast(t, w, c, I.ORIGIN, I.VS, I.MODEL_K, np.eye(4), I.MODEL_HW, 0.0, I.Z_FAR, I.VS)


def test_restatements_give_a_hostile_pixel_code_0(corner_maps):
    """Every hostile pixel has code 0 in the ICP, the colour and the point-to-SDF restatement; in the
    ICP a valid pixel whose right or lower neighbour is hostile has code 1 (no normal); the colour
    half looks at the pixel alone.  About 5 % of the frame is replaced, each dropped class at least
    five times."""
    d, hostile = H.track_frame("eye")
    md, mn, mc = corner_maps
    M = I.offset_2cm_1deg()
    assert 0.03 * d.size <= hostile.sum() <= 0.07 * d.size
    for k in np.flatnonzero(H.track_hostile(H.VALUES)):
        assert (bits(d) == bits(H.VALUES)[k]).sum() >= 5, k
    geo = I.linearize(d, H.TRACK_K, M, md, mn, I.MODEL_K, np.eye(4))
    col = C.linearize_color(d, H.track_rgb(), H.TRACK_K, M, md, mc, I.MODEL_K)
    t, w, _ = I.corner_state()
    sdf = S.linearize(d, H.TRACK_K, M, np.eye(4), t, w, **S.CORNER_VOL)
    for ref in (geo, col, sdf):
        assert (ref["code"][hostile] == 0).all() and (ref["resid"][hostile] == 0).all()
        assert np.isfinite(ref["sums"]).all() and ref["inliers"] >= 500
    with np.errstate(over="ignore"):
        good = ~H.track_hostile(d)
    nb = np.zeros_like(hostile)
    nb[:-1, :-1] = good[:-1, :-1] & (~good[:-1, 1:] | ~good[1:, :-1])
    assert nb.sum() >= 100 and (geo["code"][nb] == 1).all()
    assert (col["code"][nb] != 0).all() and (sdf["code"][nb] != 0).all()
    # the replaced pixels that stay depths are sampled like any other
    kept = (bits(d)[..., None] == bits(H.VALUES)[~H.track_hostile(H.VALUES)]).any(axis=-1)
    assert kept.sum() >= 20 and (col["code"][kept] != 0).all() and (sdf["code"][kept] != 0).all()


@pytest.mark.parametrize("name", ["ragged", "ragged_hash"])
def test_reference_tracks_on_the_hostile_frame(name):
    """The three trackers' restatements converge on the hostile frame from the first seeded start,
    with cond(A) inside what the device tests' pose-step tolerance was derived for."""
    from test_track_cpu import corner_starts
    d, _ = H.track_frame("true")
    (t, w, c), off = E.state(name)
    g = corner_starts()[0]
    md, mn, mc = R.raycast(t, w, c, I.ORIGIN, I.VS, H.TRACK_K, g, H.TRACK_HW, 0.0, I.Z_FAR, I.VS, index_offset=off)
    runs = {"icp": I.track(d, H.TRACK_K, md, mn, g),
            "rgbd": C.track(d, H.track_rgb(), H.TRACK_K, md, mn, mc, g, color_weight=E.EDGE_COLOR_WEIGHT),
            "sdf": S.track(d, H.TRACK_K, g, t, w, index_offset=off, **S.CORNER_VOL)}
    for k, r in runs.items():
        et, ea = I.pose_error(r["pose"], I.TRUE_POSE)
        print(f"{name} {k}: {r['status']} after {r['iterations']}, inliers {r['inliers'][-1]}, cond {r['cond']:.0f}, "
              f"{1e3 * et:.3f} mm / {ea:.4f} deg")
        assert r["status"] != I.LOST and r["inliers"][-1] >= 1000 and r["cond"] < 5e2
        assert np.isfinite(r["pose"]).all()
        if k != "rgbd":  # (the grey image is the textured plane's, not this model's: the colour term only has to be followed)
            assert et < 5e-3 and ea < 0.5
