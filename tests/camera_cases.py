"""Cameras with fx != fy, and cameras whose principal point lies outside the image, for the entry
points that take a camera matrix after the integrate: raycast, the ICP and RGB-D linearisations,
the three trackers, the point-to-SDF linearisation and the frustum bounds (tests/test_cameras_cpu.py
checks the conditions on these inputs with the restatements alone, tests/test_cameras_gpu.py runs the
device on them).  Plain functions and constants only; everything here runs on the CPU.  The scenes
are the corner (icp_ref) and the textured plane (icp_color_ref), both around the +z axis of the world;
a camera whose principal point is off the image looks along its own +z but sees only the rays right
of and below it, so it comes with a pose that turns its central ray onto the world's +z."""
import numpy as np

import icp_color_ref as C
import icp_ref as I

# The anisotropic pair: A_MODEL for the 83x61 model map, A_FRAME for the 71x53 frame.
A_MODEL = np.array([[118.0, 0.0, 37.6], [0.0, 86.5, 33.1], [0.0, 0.0, 1.0]])
A_FRAME = np.array([[97.0, 0.0, 30.5], [0.0, 71.0, 29.0], [0.0, 0.0, 1.0]])
# The off-image pair: anisotropic, the principal point 10.5 .. 12.2 pixels left of and above pixel
# (0, 0); the focal lengths keep the view about 37 degrees wide and high around the central ray.
OFF_MODEL = np.array([[96.0, 0.0, -11.3], [0.0, 70.0, -12.2], [0.0, 0.0, 1.0]])
OFF_FRAME = np.array([[80.0, 0.0, -11.0], [0.0, 58.0, -10.5], [0.0, 0.0, 1.0]])
TINY = ((1, 1), (5, 7), (8, 8), (3, 200), (200, 3))


def scaled(K, hw_from, hw_to):
    """K for the same view at another image size: row 0 by the width ratio, row 1 by the height ratio."""
    K = np.array(K, dtype=np.float64)
    K[0] *= hw_to[1] / hw_from[1]
    K[1] *= hw_to[0] / hw_from[0]
    return K


def swapped(K):
    """K with fx and fy exchanged (to show on the CPU that the inputs tell the two apart)."""
    K = np.array(K, dtype=np.float64)
    K[0, 0], K[1, 1] = K[1, 1], K[0, 0]
    return K


def pitch(deg):
    """A camera-to-world rotation about the origin, pitched `deg` degrees down (towards +y)."""
    a = np.radians(deg)
    P = np.eye(4)
    P[:3, :3] = [[1.0, 0.0, 0.0], [0.0, np.cos(a), np.sin(a)], [0.0, -np.sin(a), np.cos(a)]]
    return P


def aim(K, hw, eye):
    """A camera-to-world pose at `eye` whose rotation turns the ray of the image's centre onto the
    world's +z (Rodrigues about the axis perpendicular to both)."""
    c = np.array([((hw[1] - 1) / 2 - K[0, 2]) / K[0, 0], ((hw[0] - 1) / 2 - K[1, 2]) / K[1, 1], 1.0])
    c /= np.linalg.norm(c)
    ax = np.cross(c, [0.0, 0.0, 1.0])
    s = np.linalg.norm(ax)
    return I.se3(np.concatenate([ax / s * np.arctan2(s, c[2]), eye]))


# The two eyes were chosen against the restatements (seeded searches over centimetre offsets) so that
# the conditions of tests/test_cameras_cpu.py hold.  From the origin the off-image frame camera sees
# little of the corner's two side planes: the reference tracks end with cond(A) above 1e4 and 2 - 6 mm
# off; from the frame eye below cond(A) is 245 .. 297.  The model eye was then chosen for the
# linearise codes: with both cameras at one point the corner's codes 4 and 5 are rare.
OFF_FRAME_POSE = aim(OFF_FRAME, I.FRAME_HW, [0.0, 0.09, -0.07])
OFF_MODEL_POSE = aim(OFF_MODEL, I.MODEL_HW, [0.05, 0.07, -0.04])
# name -> (Kf, Km, the frame camera's pose, the model camera's pose)
PAIRS = {"aniso": (A_FRAME, A_MODEL, np.eye(4), np.eye(4)),
         "off": (OFF_FRAME, OFF_MODEL, OFF_FRAME_POSE, OFF_MODEL_POSE)}
# The second model pose of the linearise cases: the model camera (not the frame's) pitched 9 degrees
# down, so that model_pose is no identity for the "aniso" pair either and the two views still overlap.
# (track_edge_cases.pitched_model_pose() is 32 degrees: from there the 61-row model map and the 53-row
# frame share no more than a band of rows.)
MODEL_PITCH = 9.0


def lin_case(pair, pitched=False):
    """(Kf, Km, Pf, Pm, M) of a linearise case: the frame is seen from Pf, the model maps from Pm, and M
    takes the frame camera's coordinates to the model camera's after the 2 cm / 1 degree offset."""
    Kf, Km, Pf, Pm = PAIRS[pair]
    if pitched:
        Pm = pitch(MODEL_PITCH) @ Pm
    return Kf, Km, Pf, Pm, np.linalg.inv(Pm) @ I.offset_2cm_1deg() @ Pf


def lin_cases():
    """The (pair, pitched) keys of the four linearise cases."""
    return [(pair, pitched) for pair in PAIRS for pitched in (False, True)]


def track_case(pair):
    """(K, true pose, the two seeded starts) of the corner tracks (ICP and point-to-SDF): frame and
    model through the pair's frame camera, test_track_cpu's 4 cm / 2 degree starts (seed 11)."""
    Kf, _, Pf, _ = PAIRS[pair]
    true = I.TRUE_POSE @ Pf
    rng = np.random.default_rng(11)
    return Kf, true, [true @ I.perturbation(rng, 0.04, 2.0) for _ in range(2)]


def plane_track_case(pair):
    """(K, true pose, two seeded starts) of the RGB-D track on the textured plane: 2 cm / 1 degree off
    (icp_color_ref.START_SEED)."""
    Kf, _, Pf, _ = PAIRS[pair]
    true = C.TRUE_POSE @ Pf
    rng = np.random.default_rng(C.START_SEED)
    return Kf, true, [true @ I.perturbation(rng, 0.02, 1.0) for _ in range(2)]


# The every-code inputs of the point-to-SDF linearisation: through these narrower cameras the corner
# seen from the origin lies inside the volume, so the camera is pitched down until the floor plane's
# near part, in front of the volume's z = 0.5 face, is in view (code 2).
SDF_PITCH = 24.0


def sdf_code_case(pair):
    """(frame u16, K, M, G) as sdf_ref.every_code_case(): 8 cm / 3 degrees off."""
    Kf, _, Pf, _ = PAIRS[pair]
    G = pitch(SDF_PITCH) @ Pf
    return I.render(G, Kf, I.FRAME_HW), Kf, I.perturbation(np.random.default_rng(5), 0.08, 3.0), G


def lounge_raycast_cameras(K, hw=(61, 83)):
    """name -> (camera, pose names of test_raycast_gpu.poses()) for the 83x61 raycasts of the lounge
    fusion.  "aniso": the lounge intrinsics K scaled to hw, then row 1 (fy and cy) by 0.8.  The two
    poses look at the fusion's upper left, which a camera seeing only the rays right of and below its
    axis misses from "outside" (0 hits of the reference, whatever the focal lengths); so the off-image
    camera for both poses has its principal point 12 pixels right of and 10.5 above the image, and a
    narrow one with it 10.5 pixels left of and above serves "frame0" alone.  Hits of the reference on
    the oracle's fusion: aniso 2540 / 740, off-right 1138 / 1010, off-left 1914."""
    a = scaled(K, (480, 640), hw)
    a[1] *= 0.8
    return {"aniso": (a, ("frame0", "outside")),
            "off-right": (np.array([[120.0, 0.0, hw[1] + 12.0], [0.0, 90.0, -10.5], [0.0, 0.0, 1.0]]), ("frame0", "outside")),
            "off-left": (np.array([[200.0, 0.0, -10.5], [0.0, 150.0, -10.5], [0.0, 0.0, 1.0]]), ("frame0",))}


def frustum_cameras(K):
    """The two cameras of the frustum-bounds test from the lounge intrinsics K: fy at 0.8 of fx with
    the lounge's principal point, and the same with the principal point 37 / 23 pixels left of and
    above the image."""
    a = np.array(K, dtype=np.float64)
    a[1, 1] *= 0.8
    b = a.copy()
    b[0, 2], b[1, 2] = -37.25, -23.5
    return a, b


# ---- what the references reach, measured by tests/test_cameras_cpu.py (it prints every figure) --------
# Final pose errors (metres, degrees) per entry point and seeded start; every track converges, in 4 or
# 5 iterations.  cond(A): aniso icp 98 / 126, sdf 86, rgbd 211 / 198; off icp 272 / 297, sdf 245 / 251,
# rgbd 189 / 197.  The two point-to-SDF starts reach one minimum, as in test_track_sdf_cpu.py.
MEASURED = {"aniso": {"icp": [(0.547e-3, 0.0106), (0.609e-3, 0.0369)], "sdf": [(0.786e-3, 0.0212), (0.786e-3, 0.0212)],
                      "rgbd": [(1.153e-3, 0.0743), (0.524e-3, 0.0631)]},
            "off": {"icp": [(0.615e-3, 0.0544), (0.528e-3, 0.0561)], "sdf": [(0.422e-3, 0.0500), (0.422e-3, 0.0500)],
                    "rgbd": [(0.363e-3, 0.0249), (0.358e-3, 0.0275)]}}
# The lounge through factors 8 and 7.5 (64 x 80, fx 65.6, fy 70.0), the three starts of seed 23: two end
# max_iter, one converges in 10; 2370 .. 2390 inliers, cond(A) 120 .. 126.
LOUNGE_MEASURED = [(6.727e-3, 0.2110), (4.580e-3, 0.1540), (4.997e-3, 0.1583)]
# Hits of the reference raycast of the corner state at the TINY sizes (of 1, 35, 64, 600, 600 rays).
TINY_HITS = {"aniso": [1, 30, 49, 532, 549], "off": [1, 34, 52, 539, 542]}
# Codes of the reference linearisations, stride 1, and the codes a swap of fx and fy changes:
#   corner (codes 0..6; swap of Km, of Kf)          plane, colour codes 0..5 (swap of Km)
#   aniso          [292, 74, 336, 552, 161, 43, 2305]  1951 2233   [108, 717, 497, 22, 144, 2275]  1467
#   aniso pitched  [292, 74, 1068, 419, 197, 44, 1669] 1194 1693   [108, 1265, 399, 17, 144, 1830]  970
#   off            [292, 74, 394, 574, 225, 61, 2143]  2510 2745   [108, 687, 516, 34, 144, 2274]  2007
#   off pitched    [292, 74, 897, 349, 265, 57, 1829]  2101 2194   [108, 1023, 487, 48, 144, 1953] 1776
#   point-to-SDF   aniso [169, 0, 948, 334, 706, 737, 869] 1361, off [169, 0, 1589, 222, 730, 664, 389] 2117
# With the Jacobian's gradient scaling alone exchanged the 27 colour sums with a row in them move by at
# least 489 (aniso), 4852, 3388 and 3858 times the device test's bound.
