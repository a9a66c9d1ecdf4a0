"""A small fixed call pattern for a HIP API trace of one library build (TSDF_HIP_LIB selects it): one
dense and one hash handle on 128^3 at 0.08 m, 2 frames per launch; one synchronous call of 5 frames,
4 deferred frames, then a sync.  rocprofv3 --hip-trace -f csv -d DIR -- python tools/gpu/api_calls.py;
tools/gpu/api_calls_digest.py DIR names.txt then lists the calls.  Two builds that issue the same
runtime calls give the same list (profiles/r16_pipeline/)."""
import os
import sys

os.environ["TSDF_BATCH"] = "2"
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "union-thesis-slam_amd"))
import numpy as np  # noqa: E402
from tsdf_amd import grid_fusion, hash_fusion, scene  # noqa: E402

poses = scene.trajectory(9, seed=0, start=610)
d, c = scene.render(poses, scene.make_spheres(0), seed=0, start=610)
d, c = np.ascontiguousarray(d.numpy()), np.ascontiguousarray(c.numpy())
K = scene.intrinsics()
Tinv = np.linalg.inv(poses)
bnds = np.array([[0.0, 10.24]] * 3)
sums = []
for v in (grid_fusion.TSDFVolume(bnds.copy(), 0.08), hash_fusion.HashTable(bnds.copy(), 0.08, 1 << 16, max_blocks=1 << 12)):
    v.integrate_batch(d[:5], c[:5], K, Tinv[:5])
    for f in range(5, 9):
        v.integrate(c[f], d[f].astype(float) / 1000.0, K, poses[f])
    v.sync()
    T, W, C = v.get_state()
    sums.append((int((W > 0).sum()), float(W.sum()), float(C.sum())))
print("state", sums)
