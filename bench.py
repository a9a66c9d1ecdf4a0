#!/usr/bin/env python3
"""Headline benchmark: depth frames/s (and Mvoxel-updates/s) of 640x480 frames fused into a
512^3 @ 2 cm dense TSDF volume on MI355X, with the voxel-hash path measured on the same frames
(BASELINE.json metric, config[1] "1xMI355X dense grid: 1000 synthetic 640x480 frames into
512^3 @2cm"; config[2] for the hash numbers).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run does what `value` needs and no more: it generates the frames, heats the clock, runs the
W warm-up and K timed steps of the dense grid, writes the volume they left if --dump-outputs asks
(a fixed seeded sample of its voxels, DIR/<name>.npy) and prints the line.  Everything else below
(the cold window, the hash leg, ingest, drop-in, mesh, lounge and CPU-baseline legs) runs with
--full, and is null in a plain run's line.

A step is one launch's batch of frames (the unit the kernels fuse: one three-stage k_fused launch
integrates 32 frames with the brick state held in registers; TSDFVolume.frames_per_launch).  The F synthetic frames
(tsdf_amd.scene: ray-cast room with spheres seen from the BENCH_RING trajectory, mean V_f 11.7 %
of the volume; u16 millimetre depth, RGB) are generated directly in HBM before timing; W warmup
steps, then K timed steps issued asynchronously, bracketed by barrier + synchronize; the max over
ranks is taken.  With N ranks each rank owns the 8-voxel x-columns c with c % N == rank (cyclic
column shards) and integrates every frame into them -- no data-path collective --
so total work is fixed: "scaling": "strong".

Rank 0 prints ONE JSON line.  `roofline` prices the integrate launch by SURVEY §8(d)'s bytes with
temporal batching accounted for (24 B per voxel the launch's batch updates at least once, counted
on the device, + 5 B per pixel per frame) over its HIP-event time, so it cannot pass 1 by batching;
the hash leg carries the same block (+ 16 B per block looked up);
`cpu_baseline` is the NumPy restatement of the reference's CPU path (oracle/, pinned to the
reference fixtures) on a bounded sample, with the host's CPU model and BLAS threads.
Beside `value`: the hash path, the PCIe-inclusive batch rate, the reference's own per-frame
integrate() call pattern (`dropin`), and marching cubes of the fused volume.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(REPO, "union-thesis-slam_amd"), os.path.join(REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
ROOM = 10.24
VOXEL = 0.02
PIX = 640 * 480
BATCH = 32  # frames per step = frames per launch (set from the library: TSDFVolume.frames_per_launch)
WORKLOAD = "config[1]: 640x480 synthetic frames (bench ring, mean V_f 11.7%) into 512^3 @ 2 cm dense grid"
# the committed PMC passes of this round's kernel (tools/gpu/run_round_prof.sh), quoted only when
# their workload AND the build id of the library they measured match the loaded library
# (tsdf_build_id): DRAM-side traffic (FETCH_SIZE / WRITE_SIZE) and VALU issue (SQ counters)
PMC_PROFILE = os.path.join(REPO, "profiles", "pmc_integrate_r06.json")
SQ_PROFILE = os.path.join(REPO, "profiles", "pmc_sq_r06.json")
HASH_WORKLOAD = ("config[2]: the same frames into a voxel hash over the 512^3 @ 2 cm extent (8^3 blocks, 2^22 "
                 "slots, pool grown from 2^15 blocks)")
HASH_PROFILE = os.path.join(REPO, "profiles", "pmc_hash_r06.json")  # traffic + SQ of k_fused_hash<DK, true>
TEXEL_MIN_BRICKS = {"dense": 3 << 14, "hash": 3 << 15}  # Base::kTexelMinBricks* (tsdf_host.h)


def texel_dk(bricks, kind="dense"):
    """The integrate variant the library picks for a handle of `bricks` bricks (Base::texel_for):
    2 = one 8-byte depth + colour texel gather per voxel-step, 0 = a depth and a colour gather."""
    env = os.environ.get("TSDF_TEXEL")
    on = (int(env) != 0) if env is not None else bricks >= TEXEL_MIN_BRICKS[kind]
    return 2 if on else 0


def hash_owned_bricks(n):
    """Bricks a bucket-range hash shard of the bench's extent owns, about 1/n of them."""
    return (int(round(ROOM / VOXEL)) // 8) ** 3 // max(1, n)
# config[2]'s load-factor sweep (tools/hash_sweep.py), quoted only for the library build it measured
HASH_SWEEP = os.path.join(REPO, "profiles", "r06_hash_sweep.json")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one GPU each); default: the launcher's WORLD_SIZE, else 1")
    ap.add_argument("--steps", type=int, default=250,
                    help="timed steps (one launch's batch each: TSDFVolume.frames_per_launch() = 32 frames)")
    ap.add_argument("--warmup", type=int, default=12, help="untimed steps")
    ap.add_argument("--frames", type=int, default=1000, help="synthetic frames resident in HBM")
    ap.add_argument("--no-hash", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-quick", action="store_true", help="CPU baseline without the 512^3 frame")
    ap.add_argument("--no-profile", action="store_true", help="no HIP events in the timed region")
    ap.add_argument("--no-ingest", action="store_true", help="skip the host-frame (PCIe) measurement")
    ap.add_argument("--ingest-frames", type=int, default=256)
    ap.add_argument("--no-dropin", action="store_true", help="skip the per-frame integrate() measurement")
    ap.add_argument("--dropin-frames", type=int, default=256)
    ap.add_argument("--no-mesh", action="store_true", help="skip the mesh-extraction measurement")
    ap.add_argument("--no-lounge", action="store_true", help="skip the real-lounge 2 cm realism check")
    ap.add_argument("--depth-f64", action="store_true",
                    help="A/B: keep the resident depth as float64 metres (the f64-texel integrate)")
    ap.add_argument("--dist-backend", default="nccl",
                    help="nccl (RCCL, one GPU per rank) or gloo (rehearsal: several ranks may share a GPU)")
    ap.add_argument("--preheat-ms", type=float, default=300.0,
                    help="clock warm-up: untimed integrate launches on the volume (then reset) before the "
                         "W warm-up steps; 0 = none")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: the cold window, the hash leg, "
                         "host-frame ingest, drop-in calls, mesh extraction, the lounge frames and the CPU "
                         "baseline (each with its own --no-... switch); without it only the dense steps run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the volume they left (tsdf, weight, colour at a fixed "
                         "seeded sample of voxels, float32) to DIR/<name>.npy")
    ap.add_argument("--launch-selftest", action="store_true", help=argparse.SUPPRESS)  # tests: ranks, no GPU
    args = ap.parse_args()
    if not args.full:  # a plain run: set up, warm up, time the steps, print the line
        args.no_hash = args.no_cpu = args.no_ingest = args.no_dropin = args.no_mesh = args.no_lounge = True
    return args


DUMP_SAMPLE = 1 << 21  # voxels --dump-outputs keeps of each array (40 MB in all)
DUMP_SEED = 20251


def dump_outputs(vol, out_dir, rank, n):
    """--dump-outputs: what a caller of the timed path receives after its last step, the volume's
    (tsdf, weight, colour) of TSDFVolume.get_state(), at a fixed seeded sample of this rank's voxels
    (the whole 512^3 state is 1.6 GB): DIR/<name>.npy float32, and the sampled flat C-order voxel
    indices as float64 (exact below 2^53).  Ranks of a sharded run write <name>.rank<r>.npy."""
    t, w, c = vol.get_state()
    idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, t.size, size=min(DUMP_SAMPLE, t.size)))
    os.makedirs(out_dir, exist_ok=True)
    tail = f".rank{rank}" if n > 1 else ""
    for name, a in (("tsdf", t), ("weight", w), ("color", c)):
        np.save(os.path.join(out_dir, f"{name}{tail}.npy"), np.ascontiguousarray(a.reshape(-1)[idx], dtype=np.float32))
    np.save(os.path.join(out_dir, f"voxel_index{tail}.npy"), idx.astype(np.float64))


def self_launch(args):
    """`--gpus N` (N > 1) run without a launcher: start N ranks of this script under
    torch.distributed.run as a CHILD process (nothing here has touched a GPU), relay its output
    and return its exit code -- never a silent one-rank line."""
    import socket
    import subprocess
    if args.dist_backend == "nccl":
        import torch
        have = torch.cuda.device_count()  # (does not initialise the GPU on this image)
        if have < args.gpus:
            log(f"error: --gpus {args.gpus} with RCCL needs {args.gpus} GPUs, {have} visible "
                "(--dist-backend gloo rehearses several ranks on fewer GPUs)")
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    log("launching " + " ".join(cmd[1:]))
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "1"))
    return subprocess.call(cmd, env=env)


def attach_profiles(roof, st, build_id, pmc_path, sq_path, workload):
    """Attach committed PMC traffic / SQ issue profiles to a roofline block, only when they
    measured this workload with this exact library build; otherwise say why they are absent.
    pmc_path / sq_path may name the same file (the hash profile holds both)."""
    why = []
    for path, key in ((pmc_path, "traffic"), (sq_path, "valu")):
        rel = os.path.relpath(path, REPO)
        if not os.path.exists(path):
            why.append(f"{key}: no {rel}")
            continue
        with open(path) as fh:
            p = json.load(fh)
        if p.get("workload") != workload:
            why.append(f"{key}: {rel} measured another workload")
            continue
        if p.get("build_id") != build_id:
            why.append(f"{key}: {rel} measured library build {p.get('build_id')}, this is {build_id}")
            continue
        avg_s = roof["kernel_avg_us"] / 1e6
        if key == "traffic" and p.get("l2_memside_bytes_per_launch"):
            tb = float(p["l2_memside_bytes_per_launch"])
            roof["traffic"] = round(tb)
            # measured L2 memory-side bytes over this run's average launch time
            roof["traffic_frac"] = round(tb / avg_s / 1e9 / HBM_PEAK_GBS, 4)
            roof["traffic_over_algorithmic"] = round(tb / roof["bytes_per_launch"], 3)
            if p.get("raw_bytes_per_launch"):
                roof["traffic_raw"] = round(float(p["raw_bytes_per_launch"]))
            if p.get("read_requests_median"):
                roof["traffic_read_requests"] = p["read_requests_median"]
            roof["traffic_source"] = (rel + " (separate rocprofv3 --pmc passes of the same build " + build_id +
                                      ": reads = the L2's memory-side read requests by size, 32 / 64 / 128 B "
                                      "(TCC_EA0_RDREQ_*B; FETCH_SIZE tallies a 128-B request at 64 B: traffic_raw "
                                      "= FETCH_SIZE + WRITE_SIZE as reported); writes = WRITE_SIZE)")
            roof["traffic_note"] = ("L2 memory-side traffic, Infinity-Cache (256 MB) hits included, so an upper bound "
                                    "on DRAM bytes; its excess over the algorithmic bytes is the frames' depth / "
                                    "colour gathers refilled into the 4 MB per-XCD L2s by the bricks projecting "
                                    "onto them (a launch's 32 frames of images, ~48 MB, fit the Infinity Cache; "
                                    "DESIGN.md §4)")
        med = p.get("median_per_launch", {})
        if key == "valu" and med.get("SQ_INSTS_VALU"):
            vox_launch = st["voxel_updates"] / st["kernel_launches"]
            roof["valu"] = {
                "valu_busy": p["valu_busy_per_simd"],
                "valu_wave_insts_per_launch": round(med["SQ_INSTS_VALU"]),
                "valu_lane_insts_per_voxel_update": round(64.0 * med["SQ_INSTS_VALU"] / vox_launch, 1),
                "wait_any_frac": p.get("wait_any_frac"),
                "source": rel + " (rocprofv3 --pmc SQ pass of the same kernel, workload and build; busy = "
                          "SQ_ACTIVE_INST_VALU x 4 / SIMD cycles)"}
    # the binding resource: VALU issue against the HBM bytes (the algorithmic ones and the measured
    # DRAM ones; both are below peak when the SIMDs are the limit)
    v = (roof.get("valu") or {}).get("valu_busy")
    if v is not None:
        mem = max(roof["frac"], roof.get("traffic_frac") or 0.0)
        if v > mem:
            roof["bound"] = "valu"
            roof["bound_note"] = ("VALU issue-bound: the SIMDs issue VALU in valu_busy of their cycles while "
                                  "HBM moves frac (algorithmic) / traffic_frac (measured) of its peak")
    if why:
        roof["profiles_note"] = "; ".join(why)


def load_sweep(build_id, path=HASH_SWEEP):
    """BASELINE config[2]'s load-factor sweep, summarised, when the committed sweep measured this
    library build (else a note saying why it is absent)."""
    rel = os.path.relpath(path, REPO)
    if not os.path.exists(path):
        return {"note": f"no {rel}"}
    with open(path) as fh:
        p = json.loads(fh.read().strip().splitlines()[-1])
    if p.get("build_id") != build_id:
        return {"note": f"{rel} measured library build {p.get('build_id')}, this is {build_id}"}
    pts = [{"slots": q["slots"], "load_window_end": q["load_window_end"],
            "inserting_kernel_us": q["inserting"]["kernel_avg_us"],
            "inserting_over_dense": q["inserting"]["over_dense"],
            "inserting_over_load_0_1": q["inserting"].get("over_load_0_1"),
            "repeat_kernel_us": q["repeat"]["kernel_avg_us"],
            "mean_probe": q["inserting"]["mean_probe"], "max_probe": q["inserting"]["max_probe"],
            "tombstones_after": q["inserting"]["tombstones_after"]} for q in p["sweep"]]
    return {"source": rel + " (tools/hash_sweep.py, build " + build_id + ")", "workload": p.get("workload"),
            "dense_same_extent_kernel_us": p["dense_same_extent"]["async"]["kernel_avg_us"], "points": pts}


def integrate_roofline(st, frames, kernel, first_timed=None, blocks_touched=None):
    """HBM roofline of the integrate launches, priced by the bytes a launch must
    move: each voxel its batch updates at least once is read and written once (24 B: tsdf, weight,
    colour f32 in and out -- temporal batching keeps it on chip across the batch's frames), plus
    5 B per pixel per frame of input (u16 depth + RGB8), plus for the hash 16 B per block its cull
    looks up (key + slot value: one probe per kept block per launch -- a per-block count; the
    stats' bricks_touched counts z-half waves).  Counted on the device (tsdf_stats_t.batch_voxels), so `frac` cannot pass
    1 by batching.  `per_frame_bytes_frac` keeps the per-frame pricing (24 B per update per frame)
    as a secondary figure: the state traffic batching avoids."""
    if not st["kernel_launches"]:
        return None
    kernel_s = st["kernel_ms"] / 1e3
    L = st["kernel_launches"]
    avg_s = kernel_s / L
    alg = 24.0 * st["batch_voxels"] + 5.0 * PIX * frames
    per_frame = 24.0 * st["voxel_updates"] + 5.0 * PIX * frames
    if blocks_touched is not None:
        alg += 16.0 * blocks_touched
        per_frame += 16.0 * blocks_touched
    ach = alg / kernel_s / 1e9
    return {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "traffic_frac": None,
            "kernel": kernel,
            "bytes_rule": "24 B x U_batch (voxels updated at least once per launch, counted on the device) + "
                          "5 B x pixels x frames" + (" + 16 B x blocks looked up (one key + slot-value probe per "
                                                     "kept block per launch, by its cull)"
                                                     if blocks_touched is not None else ""),
            "kernel_avg_us": round(1e6 * avg_s, 2),
            "bytes_per_launch": round(alg / L),
            "batch_voxels_per_launch": round(st["batch_voxels"] / L),
            "voxel_updates_per_launch": round(st["voxel_updates"] / L),
            "per_frame_bytes_frac": round(per_frame / kernel_s / 1e9 / HBM_PEAK_GBS, 4),
            "launches": L,
            # dispatch-order index (0-based, among this process's launches of the fused kernel) of
            # the first timed integrate launch: tools/summarize_profile.py
            "first_timed_launch_index": first_timed}


def frame_ranges(start, count, F):
    """Split frames [start, start+count) of a cyclic sequence of F frames into contiguous runs."""
    out = []
    while count > 0:
        s = start % F
        n = min(count, F - s)
        out.append((s, n))
        start += n
        count -= n
    return out


# pipelined launches issued so far by run_timed (a call of n batches is n + 2 launches: the profile
# summaries find the timed integrate launches in a kernel trace by this count)
LAUNCHES = {"issued": 0}


def run_timed(vol, depth, rgb, K, Tinv, start, count, F, sync, barrier, profile, async_=True):
    """Issue `count` frames (asynchronously unless async_=False); returns wall seconds."""
    from tsdf_amd import _ffi
    dptr, cptr = depth.data_ptr(), rgb.data_ptr()
    dstride, cstride = depth[0].numel() * depth.element_size(), rgb[0].numel()
    dk = _ffi.DEPTH_F64_M if depth.element_size() == 8 else _ffi.DEPTH_U16_MM
    hw = tuple(depth.shape[1:3])
    vol.set_profiling(profile)
    vol.stats(reset=True)
    barrier()
    sync()
    t0 = time.perf_counter()
    for s, n in frame_ranges(start, count, F):
        vol.integrate_batch(dptr + s * dstride, cptr + s * cstride, K, Tinv[s:s + n], hw=hw,
                            device_ptrs=True, sync=not async_, depth_kind=dk)
        LAUNCHES["issued"] += (n + BATCH - 1) // BATCH + 2
    vol.sync()
    sync()
    return time.perf_counter() - t0


def cpu_info():
    model = None
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    blas = []
    try:
        from threadpoolctl import threadpool_info
        blas = [{"api": d.get("internal_api"), "threads": d.get("num_threads")} for d in threadpool_info()
                if d.get("user_api") == "blas"]
    except Exception:
        pass
    return model, blas


def cpu_baseline(depth, rgb, poses, K, first):
    """The reference's CPU path restated in NumPy (oracle.numpy_port_integrate, the per-voxel
    hash loop oracle.NumpyPortHash), pinned bit-exact to the reference fixtures by
    tests/test_oracle_golden.py, timed on this host on a bounded sample."""
    import oracle as O
    model, blas = cpu_info()
    threads = max([b["threads"] or 1 for b in blas] or [1])
    res = {"unit": "frames/s", "kind": "port", "cpu_model": model, "host_cpus": os.cpu_count(),
           "blas": blas, "cores": threads,
           "cores_note": "NumPy elementwise passes run on one core; np.dot (rigid_transform) uses the "
                         "BLAS threads listed"}
    # config[0]: lounge frame 0 -> 128^3 @ 4 cm, median of 7
    d0, c0, p0, K0 = O.lounge_frame(0)
    c1 = np.array([[-2.56, 2.56], [-2.56, 2.56], [0.0, 5.12]])
    vol = O.OracleTSDFVolume(c1.copy(), 0.04)
    coords = O.vox_coords_for(vol._vol_dim)
    ts = []
    for _ in range(7):
        vol = O.OracleTSDFVolume(c1.copy(), 0.04)
        t0 = time.perf_counter()
        n0 = O.numpy_port_integrate(vol, coords, c0, d0, K0, p0)
        ts.append(time.perf_counter() - t0)
    res["config0"] = {"s_per_frame_median": round(float(np.median(ts)), 4), "voxels_updated": n0,
                      "sample": "lounge frame-000000 into 128^3 @ 4 cm, median of 7 (grid_fusion.py:214-314)"}
    # hash: the per-voxel loop (hash_fusion.py:134-145) on the same frame
    hp = O.NumpyPortHash(c1.copy(), 0.04, 1000000)
    t0 = time.perf_counter()
    nh = hp.integrate(coords, c0, d0, K0, p0)
    th = time.perf_counter() - t0
    res["hash_mvox_updates_per_s"] = round(nh / th / 1e6, 5)
    res["hash_sample"] = f"lounge frame-000000 at 128^3 @ 4 cm: {nh} per-voxel updates in {th:.2f} s"
    # the bench's own workload: one synthetic frame into the full 512^3 @ 2 cm volume
    res["value"] = round(1.0 / float(np.median(ts)), 4)
    res["sample"] = "config[0] only (--cpu-quick)"
    if depth is not None:
        big = O.OracleTSDFVolume(np.array([[0.0, ROOM]] * 3), VOXEL)
        coords = O.vox_coords_for(big._vol_dim)
        d = depth.astype(float) / 1000.0
        t0 = time.perf_counter()
        n = O.numpy_port_integrate(big, coords, rgb, d, K, poses)
        tb = time.perf_counter() - t0
        res["value"] = round(1.0 / tb, 5)
        res["sample"] = (f"synthetic frame {first} into the full 512^3 @ 2 cm volume, {n} voxels updated, "
                         f"{tb:.1f} s (vox_coords built untimed, as the reference's constructor does)")
        res["mvox_updates_per_s"] = round(n / tb / 1e6, 3)
        del coords, big
    return res


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    if "WORLD_SIZE" not in os.environ and (args.gpus or 1) > 1:
        sys.exit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus is None:  # a launcher without --gpus: its WORLD_SIZE
        args.gpus = world
    if args.gpus != world:
        log(f"error: --gpus {args.gpus} but the launcher started WORLD_SIZE {world} ranks")
        sys.exit(2)
    n = world
    if args.launch_selftest:  # the launch path alone (CPU tests): ranks meet over gloo, no GPU
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"selftest": True, "n_gpus": n, "ranks_seen": int(t.item())}), flush=True)
        dist.destroy_process_group()
        return
    gpu = local if args.dist_backend == "nccl" else local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    if n > 1:
        # the backends' connection messages go to fd 1 (gloo prints "Rank r is connected to ...");
        # send them to stderr so that stdout carries only the JSON line
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.dist_backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group(args.dist_backend)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
    red_dev = dev if args.dist_backend == "nccl" else torch.device("cpu")

    def barrier():
        if n > 1:
            dist.barrier()

    def sync():
        torch.cuda.synchronize()

    def reduce(x, op):
        if n == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=op)
        return float(t.item())

    def max_over_ranks(x):
        return reduce(x, dist.ReduceOp.MAX if n > 1 else None)

    def sum_over_ranks(x):
        return reduce(x, dist.ReduceOp.SUM if n > 1 else None)

    from tsdf_amd import _ffi, grid_fusion, hash_fusion, scene

    # ---- synthetic workload, generated in HBM ---------------------------------------------
    F = args.frames
    t0 = time.perf_counter()
    poses = scene.trajectory(F, seed=0, radius_frac=scene.BENCH_RING)
    spheres = scene.make_spheres(0, ring_frac=scene.BENCH_RING)
    depth = torch.empty((F, 480, 640), dtype=torch.int16, device=dev)
    rgb = torch.empty((F, 480, 640, 3), dtype=torch.uint8, device=dev)
    for s in range(0, F, 50):
        d, c = scene.render(poses[s:s + 50], spheres, seed=0, start=s, device=dev, depth_dtype=torch.int16)
        depth[s:s + len(d)] = d
        rgb[s:s + len(c)] = c
    Tinv = np.ascontiguousarray(np.linalg.inv(poses))
    K = scene.intrinsics()
    if args.depth_f64:  # NumPy's f64(u16) / 1000: the same metres the u16 path computes
        depth = torch.from_numpy(depth.cpu().numpy().view(np.uint16).astype(np.float64) / 1000.0).to(dev)
    sync()
    log(f"[rank {rank}] generated {F} frames in HBM in {time.perf_counter() - t0:.1f}s")

    # ---- dense grid: this rank's columns of 512^3 @ 2 cm ----------------------------------
    X = int(round(ROOM / VOXEL))
    bnds = np.array([[0.0, ROOM]] * 3)
    with contextlib.redirect_stdout(sys.stderr):  # the reference-style ctor prints; keep stdout JSON-only
        vol = grid_fusion.TSDFVolume(bnds, VOXEL, device=gpu, shard=(rank, n))
    global BATCH
    BATCH = vol.frames_per_launch()  # a step = one launch's temporal batch (32 frames)
    W, Ks = args.warmup, args.steps
    Wf, Kf = W * BATCH, Ks * BATCH
    cold = None
    if args.preheat_ms > 0:
        # Clock warm-up.  After the frame generation the GPU runs below its steady clock, and it
        # takes it tens of milliseconds of load to get there: the driver's --steps 20 window (13 ms at
        # round 4's 16-frame steps) measured cold read ~13 % low (profiles/r04_clock/).  So the window is measured once
        # cold (reported as cold_window), then the integrate runs untimed for preheat_ms, the
        # volume is reset, and the W warm-up and K timed steps run as always.  (The cold reading
        # is a measurement of its own: --full.)
        if args.full:
            run_timed(vol, depth, rgb, K, Tinv, 0, Wf, F, sync, barrier, False)
            cdt = max_over_ranks(run_timed(vol, depth, rgb, K, Tinv, Wf, Kf, F, sync, barrier, not args.no_profile))
            cst = vol.stats()
            cold = {"frames_per_s": round(Kf / cdt, 1),
                    "kernel_avg_us": round(1e3 * cst["kernel_ms"] / max(1, cst["kernel_launches"]), 2),
                    "note": f"the same window on a fresh volume before the clock warm-up ({args.preheat_ms:.0f} ms of "
                            f"untimed integrate launches, then a reset)"}
        t_end = time.perf_counter() + args.preheat_ms / 1e3
        f0 = Wf + Kf
        while time.perf_counter() < t_end:
            run_timed(vol, depth, rgb, K, Tinv, f0, 20 * BATCH, F, sync, lambda: None, False)
            f0 += 20 * BATCH
        vol.reset()
        barrier()
    run_timed(vol, depth, rgb, K, Tinv, 0, Wf, F, sync, barrier, False)
    first_timed = LAUNCHES["issued"] + 2  # (the timed call's first two launches fill the pipeline)
    dt = run_timed(vol, depth, rgb, K, Tinv, Wf, Kf, F, sync, barrier, not args.no_profile)
    st = vol.stats()
    if args.dump_outputs:  # before any side leg integrates further into the volume
        t0 = time.perf_counter()
        dump_outputs(vol, args.dump_outputs, rank, n)
        log(f"[rank {rank}] wrote the sampled volume to {args.dump_outputs} in {time.perf_counter() - t0:.1f}s")
    dt_max = max_over_ranks(dt)
    vox = sum_over_ranks(float(st["voxel_updates"]))
    fps = Kf / dt_max
    kernel_s = st["kernel_ms"] / 1e3
    local_bricks = int(np.prod((np.asarray(vol._local_dim) + 7) // 8))
    roof = integrate_roofline(st, Kf, f"tsdf::k_fused<true, 4, {texel_dk(local_bricks)}, true>: integrates batch k "
                                      "(and culls k+1, preps k+2 in the same launch)", first_timed)
    if roof is not None:
        attach_profiles(roof, st, _ffi.build_id(), PMC_PROFILE, SQ_PROFILE, WORKLOAD)
    vf_mean = st["voxel_updates"] / Kf
    log(f"[rank {rank}] dense: {Kf} frames in {dt * 1e3:.1f} ms -> {Kf / dt:.0f} frames/s, "
        f"V_f mean {vf_mean:.0f} ({100 * vf_mean / (len(vol.x_index) * X * X):.1f}% of shard), "
        f"kernel {st['kernel_ms']:.1f} ms over {st['kernel_launches']} launches, "
        f"bricks visited/frame {st['bricks_visited'] / Kf:.0f}, touched/frame {st['bricks_touched'] / Kf:.0f}")
    dense_bytes = 3 * 4 * len(vol.x_index) * X * X
    # side legs that fail are reported in the line's top-level "errors" (every rank's), never
    # silently: the throughput measurement above stands either way
    errors = []
    # ---- PCIe-inclusive rate: the same frames from pageable host memory (not `value`) -------
    ingest = None
    if not args.no_ingest:
        ni = min(args.ingest_frames, F)
        dh = depth[:ni].cpu().numpy().view(np.uint16)
        ch = rgb[:ni].cpu().numpy()
        vol.set_profiling(False)
        # one untimed launch's worth first: the handle allocates its page-locked bounce slots and
        # device staging slots at its first host-frame call (a one-time cost, not the rate)
        vol.integrate_batch(dh[:BATCH], ch[:BATCH], K, Tinv[:BATCH], sync=True)
        barrier()
        sync()
        t0 = time.perf_counter()
        vol.integrate_batch(dh, ch, K, Tinv[:ni], sync=True)
        ti = max_over_ranks(time.perf_counter() - t0)
        ingest = {"frames_per_s": round(ni / ti, 1), "frames": ni,
                  "source": "pageable numpy arrays copied by host threads into page-locked bounce "
                            "slots, DMA on a copy stream into four device staging slots, overlapped "
                            "with the pipelined launches (tsdf_dense_integrate_batch without "
                            "TSDF_DEVICE_PTRS)"}
        log(f"[rank {rank}] ingest: {ni} host frames in {ti * 1e3:.1f} ms -> {ni / ti:.0f} frames/s")
    # ---- N > 1: host frames ingested once on rank 0 and broadcast over RCCL ---
    bcast = None
    if not args.no_ingest and n > 1:
        from tsdf_amd import sharding
        try:
            ni = min(args.ingest_frames, F)
            dh = depth[:ni].cpu().numpy().view(np.uint16) if rank == 0 else None
            ch = rgb[:ni].cpu().numpy() if rank == 0 else None
            vol.set_profiling(False)
            barrier()
            sync()
            t0 = time.perf_counter()
            sharding.integrate_broadcast(vol, K, dh, ch, Tinv[:ni] if rank == 0 else None)
            tb = max_over_ranks(time.perf_counter() - t0)
            be = dist.get_backend()
            bcast = {"frames_per_s": round(ni / tb, 1), "frames": ni, "backend": be,
                     "source": f"rank 0's host frames, pinned H2D once, broadcast to every rank in chunks "
                               f"of 64 over {'RCCL' if be == 'nccl' else be} in {sharding._device().type} "
                               f"buffers (sharding.integrate_broadcast), integrated while the next chunk travels"}
            log(f"[rank {rank}] broadcast ingest: {ni / tb:.0f} frames/s")
        except Exception as e:  # reported (top-level "errors"), never fatal to the throughput measurement
            bcast = {"error": f"{type(e).__name__}: {e}"[:300]}
            errors.append(f"broadcast_ingest, rank {rank}: " + bcast["error"])
            log(f"[rank {rank}] broadcast ingest failed: {e}")
    # ---- mesh extraction of the fused volume (not part of `value`) ----
    mesh = None
    if not args.no_mesh and n > 1:
        # sharded marching cubes: border rows traded point to point (RCCL over xGMI), then each
        # rank meshes the cells anchored at its own columns (tsdf_amd.sharding.mesh_shard)
        from tsdf_amd import sharding
        try:
            barrier()
            sync()
            t0 = time.perf_counter()
            part = sharding.mesh_shard(vol)
            sync()
            tm = max_over_ranks(time.perf_counter() - t0)
            mesh = {"ms": round(1e3 * tm, 2), "triangles": int(sum_over_ranks(len(part[1]))),
                    "vertices_with_border_copies": int(sum_over_ranks(len(part[0]))),
                    "note": "per-shard marching cubes with the neighbours' border rows (point-to-point "
                            "exchange + extraction, max over ranks); the union is the unsharded mesh"}
            log(f"[rank {rank}] sharded mesh: {len(part[1])} triangles in {tm * 1e3:.1f} ms")
        except Exception as e:  # reported (top-level "errors"), never fatal to the throughput measurement
            mesh = {"error": f"{type(e).__name__}: {e}"[:300]}
            errors.append(f"sharded mesh, rank {rank}: " + mesh["error"])
            log(f"[rank {rank}] sharded mesh failed: {e}")
    if not args.no_mesh and rank == 0 and n == 1:
        import ctypes
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        sync()
        t0 = time.perf_counter()
        _ffi.call("tsdf_dense_extract_mesh", vol._h, ctypes.byref(nv), ctypes.byref(nt))
        tm = time.perf_counter() - t0
        mesh = {"ms": round(1e3 * tm, 2), "vertices": nv.value, "triangles": nt.value,
                "mvoxels_per_s": round(X ** 3 / tm / 1e6, 1),
                "note": "marching cubes on the device over the fused 512^3 volume after the timed run"}
        log(f"[rank {rank}] mesh: {nv.value} vertices, {nt.value} triangles in {tm * 1e3:.1f} ms")
    vol.close()
    del vol
    torch.cuda.empty_cache()

    # ---- voxel hash on the same frames (config[2]: 8^3 blocks, 2^22 buckets) ---------------
    hash_res = None
    if not args.no_hash:
        with contextlib.redirect_stdout(sys.stderr):
            # pool sized for the live blocks, not the extent: it starts at 2^15 blocks and grows
            # (synchronously in the warmup, ahead of the launches in the asynchronous timed run)
            ht = hash_fusion.HashTable(np.array([[0.0, ROOM]] * 3), VOXEL, 1 << 22, device=gpu,
                                       max_blocks=1 << 15, shard=rank, n_shards=n)
        run_timed(ht, depth, rgb, K, Tinv, 0, Wf, F, sync, barrier, False, async_=False)
        hdt = run_timed(ht, depth, rgb, K, Tinv, Wf, Kf, F, sync, barrier, not args.no_profile)
        hs = ht.stats()
        peak_pool = ht.info()["pool_capacity"]
        # the same window again on the table it left (every block exists: lookups only, no
        # allocation) -- separates the timed window's insert cost from the steady-state cost
        hdt2 = run_timed(ht, depth, rgb, K, Tinv, Wf, Kf, F, sync, barrier, not args.no_profile)
        hs2 = ht.stats()
        ht.trim()  # the run's end: the pool hands the memory above its live blocks back
        info = ht.info()
        if hs["bricks_skipped"]:
            raise RuntimeError(f"hash table/pool overflowed ({hs['bricks_skipped']} bricks skipped)")
        hdt_max = max_over_ranks(hdt)
        hvox = sum_over_ranks(float(hs["voxel_updates"]))
        used = sum_over_ranks(info["used"])
        hash_bytes = info["slots"] * (8 + 4) + info["pool_capacity"] * (3 * 4 * 512 + 64 + 4)
        hash_res = {"frames_per_s": round(Kf / hdt_max, 1),
                    "mvox_updates_per_s": round(hvox / hdt_max / 1e6, 1),
                    "ms_per_step": round(1e3 * hdt_max / Ks, 4),
                    "buckets": 1 << 22, "block": "8^3",
                    "load_factor": round(used / (1 << 22), 4),
                    "blocks_live": int(used),
                    "pool_capacity": int(sum_over_ranks(info["pool_capacity"])),
                    "pool_capacity_in_run": int(sum_over_ranks(peak_pool)),
                    "mean_probe": round(hs["probe_steps"] / max(1, hs["lookups"]), 3),
                    "max_probe": int(hs["probe_max"]),
                    "kernel_avg_us": round(1e3 * hs["kernel_ms"] / max(1, hs["kernel_launches"]), 2),
                    "blocks_allocated_in_window": int(hs["blocks_allocated"]),
                    "no_alloc_repeat": {"frames_per_s": round(Kf / max_over_ranks(hdt2), 1),
                                        "kernel_avg_us": round(1e3 * hs2["kernel_ms"] / max(1, hs2["kernel_launches"]), 2),
                                        "blocks_allocated": int(hs2["blocks_allocated"]),
                                        "note": "the same timed window integrated again into the table it left "
                                                "(every updated block exists; the culls still insert, and the call's end "
                                                "frees, the few kept bricks no frame updates: blocks_allocated); not the "
                                                "headline"},
                    "hbm_state_bytes": int(sum_over_ranks(hash_bytes)),
                    "dense_hbm_state_bytes": int(sum_over_ranks(dense_bytes)),
                    "state_bytes_note": "hash: table keys + slot->block map + block pool (tsdf/weight/"
                                        "colour, entry bits, free list) after the run (HashTable.trim; "
                                        "pool_capacity_in_run: before it, with the growth headroom of the "
                                        "launches in flight); dense: three f32 arrays of the volume",
                    "roofline": None}
        hroof = integrate_roofline(hs, Kf, f"tsdf::k_fused_hash<{texel_dk(hash_owned_bricks(n), 'hash')}, true>: integrates "
                                           "batch k (find-or-insert of its "
                                           "blocks), culls k+1 and preps k+2 in the same launch; the window "
                                           "inserts blocks_allocated_in_window blocks",
                                   blocks_touched=hs["lookups"])
        if hroof is not None:
            attach_profiles(hroof, hs, _ffi.build_id(), HASH_PROFILE, HASH_PROFILE, HASH_WORKLOAD)
            hash_res["roofline"] = hroof
        hash_res["load_sweep"] = load_sweep(_ffi.build_id())
        log(f"[rank {rank}] hash: {Kf / hdt:.0f} frames/s, load {hash_res['load_factor']}, "
            f"pool {info['pool_capacity']} blocks for {info['used']} live")
        ht.close()
        del ht
        torch.cuda.empty_cache()

    # ---- the reference's call pattern: one integrate() per host frame (drop-in) -------------
    dropin = None
    if not args.no_dropin and n == 1:
        nd = min(args.dropin_frames, F)
        d64 = depth[:nd].cpu().numpy().view(np.uint16).astype(np.float64) / 1000.0  # as grid_demo1.py:81
        ch = rgb[:nd].cpu().numpy()
        dropin = {"frames": nd, "call": "TSDFVolume.integrate(color_im u8, depth_im f64 m, K, pose) / "
                                        "HashTable.integrate per frame from host numpy, then get_volume's "
                                        "flush (grid_demo1.py:76-87, hash_demo1.py:39)"}
        for name, mk in (("dense", lambda: grid_fusion.TSDFVolume(np.array([[0.0, ROOM]] * 3), VOXEL, device=gpu)),
                         ("hash", lambda: hash_fusion.HashTable(np.array([[0.0, ROOM]] * 3), VOXEL, 1 << 22,
                                                                device=gpu, max_blocks=1 << 15))):
            with contextlib.redirect_stdout(sys.stderr):
                v = mk()
            v.integrate(ch[0], d64[0], K, poses[0])  # first call allocates the staging slots
            v.sync()
            rates = []
            for _ in range(3):  # three passes over the frames (host-side timing is noisy): the median
                t0 = time.perf_counter()
                for i in range(1, nd):
                    v.integrate(ch[i], d64[i], K, poses[i])
                v.sync()
                rates.append(round((nd - 1) / (time.perf_counter() - t0), 1))
            dropin[name + "_frames_per_s"] = sorted(rates)[1]
            dropin[name + "_passes"] = rates
            v.close()
            log(f"[rank {rank}] drop-in {name}: {sorted(rates)[1]:.0f} frames/s per-frame integrate() {rates}")
        with contextlib.redirect_stdout(sys.stderr):
            v = grid_fusion.TSDFVolume(np.array([[0.0, ROOM]] * 3), VOXEL, device=gpu, defer=False)
        nu = min(64, nd)
        v.integrate(ch[0], d64[0], K, poses[0])
        t0 = time.perf_counter()
        for i in range(1, nu):
            v.integrate(ch[i], d64[i], K, poses[i])
        tu = time.perf_counter() - t0
        dropin["dense_undeferred_frames_per_s"] = round((nu - 1) / tu, 1)
        v.close()
        del d64, ch
        torch.cuda.empty_cache()

    # ---- realism check: the real lounge frames at 2 cm ------------------
    lounge = None
    if not args.no_lounge and n == 1:
        from PIL import Image
        root = os.path.join(REPO, "tests", "golden", "lounge")
        nl = 10  # the depth frames committed with the tests (frames 0-9; colour for 0-2)
        ld = np.stack([np.array(Image.open(os.path.join(root, "frame-%06d.depth.png" % i))) for i in range(nl)])
        lc = np.zeros(ld.shape + (3,), np.uint8)
        for i in range(3):
            lc[i] = np.array(Image.open(os.path.join(root, "frame-%06d.color.jpg" % i)).convert("RGB"))
        lp = np.stack([np.loadtxt(os.path.join(root, "frame-%06d.pose.txt" % i)) for i in range(nl)])
        lK = np.loadtxt(os.path.join(root, "camera-intrinsics.txt"), delimiter=" ")
        reps = 40  # the 10 frames cycled: 400 frames
        dd = torch.from_numpy(np.ascontiguousarray(np.tile(ld, (reps, 1, 1)).astype(np.uint16).view(np.int16))).to(dev)
        cc = torch.from_numpy(np.ascontiguousarray(np.tile(lc, (reps, 1, 1, 1)))).to(dev)
        lT = np.ascontiguousarray(np.tile(np.linalg.inv(lp), (reps, 1, 1)))
        lb = np.array([[-4.22106438, 3.86798203], [-2.6663104, 2.60146141], [0., 5.76272371]])  # hash_map_test.py:11
        with contextlib.redirect_stdout(sys.stderr):
            lv = grid_fusion.TSDFVolume(lb, VOXEL, device=gpu)
        lv.integrate_batch(dd.data_ptr(), cc.data_ptr(), lK, lT[:40], hw=(480, 640), device_ptrs=True,
                           invalid_65535=True)
        lv.stats(reset=True)
        sync()
        t0 = time.perf_counter()
        lv.integrate_batch(dd.data_ptr(), cc.data_ptr(), lK, lT, hw=(480, 640), device_ptrs=True, sync=False,
                           invalid_65535=True)
        lv.sync()
        tl = time.perf_counter() - t0
        ls = lv.stats()
        lounge = {"frames_per_s": round(len(lT) / tl, 1), "frames": len(lT),
                  "mvox_updates_per_s": round(ls["voxel_updates"] / tl / 1e6, 1),
                  "mean_voxels_updated_per_frame": round(ls["voxel_updates"] / len(lT)),
                  "volume": "405x264x289 @ 0.02 m (lounge bounds, hash_map_test.py:11)",
                  "source": "tests/golden/lounge frames 0-9 (u16 PNG depth, 65535 masked on the device), "
                            "cycled 40 times from HBM"}
        log(f"[rank 0] lounge 2 cm: {len(lT) / tl:.0f} frames/s, V_f {ls['voxel_updates'] / len(lT):.0f}")
        lv.close()
        del dd, cc

    # ---- CPU baseline: the NumPy restatement of the reference CPU path --------------------
    cpu = None
    if rank == 0 and n == 1 and not args.no_cpu:
        f0 = Wf % F
        dh = None if args.cpu_quick else depth[f0].cpu().numpy().view(np.uint16)
        ch = None if args.cpu_quick else rgb[f0].cpu().numpy()
        t0 = time.perf_counter()
        cpu = cpu_baseline(dh, ch, poses[f0], K, f0)
        log(f"[rank 0] cpu baseline: {cpu['value']} frames/s ({time.perf_counter() - t0:.1f} s)")

    if n > 1:  # every rank's side-leg failures, on rank 0
        every = [None] * n
        dist.all_gather_object(every, errors)
        errors = [e for part in every for e in part]
    if errors:
        log("SIDE-LEG ERRORS: " + " | ".join(errors))
    if rank == 0:
        line = {
            "metric": "depth frames/sec (640x480 into 512^3 @ 2 cm dense TSDF; hash alongside)",
            "value": round(fps, 1), "unit": "frames/s", "n_gpus": n, "steps": Ks, "warmup": W, "full": args.full,
            "ms_per_step": round(1e3 * dt_max / Ks, 4), "frames_per_step": BATCH,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "build_id": _ffi.build_id(),
            "data": "synthetic (ray-cast 10.24 m room + spheres, u16 mm depth, RGB8; generated in HBM)",
            "config": {"workload": WORKLOAD, "volume": "512x512x512 @ 0.02 m", "frames_resident": F,
                       "image": "640x480", "timed_frames": Kf,
                       "parallelism": f"cyclic 8-voxel x-columns over {n} ranks" if n > 1 else "single GPU"},
            "mvox_updates_per_s": round(vox / dt_max / 1e6, 1),
            "mean_voxels_updated_per_frame": round(vox / Kf),
            "clock_warmup_ms": args.preheat_ms,
            "cold_window": cold,
            # (dispatch-order index of the first timed integrate launch, also without --profile)
            "first_timed_launch_index": first_timed,
            "hash": hash_res,
            "pcie_inclusive": ingest,
            "broadcast_ingest": bcast,
            "dropin": dropin,
            "lounge_2cm": lounge,
            "mesh": mesh,
            "roofline": roof,
            "cpu_baseline": cpu,
            "errors": errors,
        }
        print(json.dumps(line), flush=True)
    if n > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
