#!/usr/bin/env python3
"""bench.py — Mray/s (primary+bounce) of the Renderer::Accumulate hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Workload, for every N (BASELINE.json configs[3], "cfg4", SURVEY.md §8d — the config the metric is quoted on): the fixed
4096x4096 image of the synthetic scene S(100000) (ground + 99 999 random spheres, 17 materials, 1562 emissive spheres,
ambient 0), SAH BVH, MIS on, Policy.max_bounces = 9 (primary + 8 bounces).  One STEP = 64 x Renderer::Accumulate() over
that image.  N = 1 renders the whole image on one GPU; N > 1 splits its tile rows over the ranks (interleaved rows,
Renderer.hpp:75 is the axis being split): STRONG scaling, no data-path collective, one RCCL gather of the accumulator
slabs after the timed region (timed separately).  --config cfg2|cfg3|cfg5 selects the other BASELINE configs, same rules.

value = rays handed to closest-hit traversal by all ranks (Renderer.hpp:165: primary + extension rays; shadow rays are
reported separately) / max-over-ranks wall time of the K timed steps, inputs resident in HBM, no profiling in that pass.

A plain run does only that: set-up, W warm-up steps, the K timed steps (and the gather for N > 1), the JSON line.  --full adds
everything else the line can carry (null without it): the roofline passes and rocprofv3 --pmc child passes below,
value_with_every_primary_ray_walking_the_tree, kernel_ms_per_step, shadow_rays_per_step, the CPU baseline and, for N > 1, group_host.
--no-counts / --no-pmc / --no-cpu-baseline / --no-group-host leave out parts of a --full run.

--dump-outputs DIR writes what the timed path leaves for its caller after the last timed step: the accumulator ([tile][bucket][rgb][256]
f32, Renderer.hpp:43-46; for N > 1 the gathered image) as DIR/accumulator_tiles.npy (float32, a fixed sample of whole tiles, drawn with
seed 0, in ascending tile order) and DIR/accumulator_tile_sums.npy (float64 [tile][rgb], every tile's radiance summed over buckets and
pixels).  The inputs are fixed by the arguments, so two builds can be compared output for output.

roofline (--full; rank 0's share of the image for N > 1): k_trace, the dominant kernel, is bound by VALU issue, not by HBM (its BVH bytes are
served from LDS/L2; north_star's ">= 60 % of the HBM roofline" does not apply to a cache-resident tree — roofline.hbm carries the §8d
figure and the measured traffic as labelled secondaries).
  * per-kernel durations: HIP events on the launch stream, in a second live pass with one batch in flight (policy.profile);
  * VALU instructions, lane utilisation and HBM bytes (FETCH_SIZE / WRITE_SIZE): measured IN THIS RUN by short child
    processes of this script under `rocprofv3 --pmc` (one batch each, separate passes as MI355X_MICROARCH.md prescribes),
    started by rank 0 before it touches the GPU or joins the process group.  Where rocprofv3 is unavailable those fields are null.
  * roofline.frac = useful_lane_frac: VALU-issuing SIMD-cycles x the share of lanes doing work in them, over all SIMD-cycles;
    issue_frac (lanes not weighed) and arithmetic_frac (slab-test and sphere-test lane-operations against the all-FMA vector peak) beside it.

--group: the other host of the multi-GPU path — ONE process drives --gpus N devices through the library's mirt_group_* entry points
(in-library RCCL gather); same workload and JSON line, no roofline / CPU legs.  Under torch.distributed.run, rank 0 also runs it once as a
child process after the ranks have released their GPUs and reports it as `group_host` (gather_ms of both hosts in one driver command).
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
# VALU roof.  The resource is the SIMD's vector ALU issue: 256 CUs x 4 SIMDs = 1024 pipes, one issue slot per quad-cycle each.
#   achieved = VALU-issuing quad-cycles x 4 per second, from this run's PMC child pass: SQ_INSTS_VALU - SQ_ACTIVE_INST_VALU2 (the
#              quad-cycles in which two VALU instructions issued together hold two instructions) per traced ray x rays traced per second;
#   peak     = 1024 SIMDs x 2.4 GHz max clock; frac = share of all SIMD-cycles in which the VALU was issuing for this kernel.
# Why not lane-instructions against the 78.6 Tlane-inst/s behind the 157.3 TFLOP/s vector peak (kept as `lane_instructions`): only
# plain f32 add / mul / fma reach that rate.  Measured with 8 waves per SIMD (profiles/experiments/valu_rates.hip, profiles/r02/valu_rates.txt):
# v_fma_f32 2.6, v_add_f32 2.5, v_fma_mix_f32 4.4, v_med3 / v_max3 / v_max / v_lshl_add 4.3, v_cmp + v_cndmask 3.3 each, v_sqrt_f32 8.2
# cycles per wave64 instruction.  k_trace's traversal step is ~80 % such half-rate work (compares, selects, min / max / med3,
# binary16-decoding FMAs, integer address arithmetic): the all-FMA rate is not reachable by a traversal, the issue slots are.
VALU_PEAK_GCYC = 256 * 4 * 2.4            # 10^9 SIMD-cycles per second
VALU_PEAK_TLANE = 256 * 4 * 32 * 2.4e9 / 1e12
# arithmetic_frac: the lane-operations a traversal is FOR — slab tests and sphere tests — against the all-FMA vector peak.  Static VALU
# counts from the ISA listing (`make -C cpu-raytracing-experiments_amd/csrc asm`, profiles/r03/static_counts.txt): one child box of a 4-wide record =
# 6 v_fma_mix + 3 v_med3 + 3 v_max3 (per-axis enter / leave) + v_max(0) + v_min(tfar) + v_max3 + v_min3 + v_cmp = 17; one closest-hit
# sphere test (intersect_prims, FMA chain + correctly rounded sqrt + the (dist, index) acceptance) = 31; one any-hit sphere test = 32.
# Dynamic counts: the kernels' own box / sphere counters (policy.count_traffic), equal to the CPU twin's.
OPS_PER_BOX, OPS_PER_SPHERE, OPS_PER_SHADOW_SPHERE = 17, 31, 32
DUMP_SAMPLE_TILES, DUMP_SAMPLE_BYTES = 1024, 56 << 20    # --dump-outputs: at most this many whole tiles / bytes of accumulator words
MIX_COUNTERS = "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU2 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_CVT"
SQ_COUNTERS = "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAIT_ANY"


def algorithmic_bytes(c):
    """SURVEY.md §8d, for the k_trace launches (closest-hit rays of bounce b + shadow rays of bounce b-1 in one kernel):
    per closest-hit ray 24 B (p,dir) + 12 B (tfar,primID,matID) + 32 B per BVH child box tested + 32 B per sphere tested;
    per shadow ray 28 B (p,dir,tfar) + 1/8 B (occluded bit) + 32 B per box + 32 B per sphere."""
    return (36 * c["rays"] + 32 * (c["nodes"] + c["spheres"])
            + 28.125 * c["shadow_rays"] + 32 * (c["shadow_nodes"] + c["shadow_spheres"]))


def load_mirt():
    return importlib.import_module("cpu-raytracing-experiments_amd")


def make_renderer(mirt, cfg, device, **kw):
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    return mirt.Renderer(sc, device=device, max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], mis=True, use_bvh=bool(cfg["use_bvh"]), **kw)


# ---- child process under rocprofv3 --pmc: one batch, one kernel on the GPU at a time ------------------------------------
def pmc_child(args):
    mirt = load_mirt()
    cfg = dict(mirt.scene.CONFIGS[args.config])
    r = make_renderer(mirt, cfg, 0, streams=1, max_batch=args.max_batch)
    r.Resize(cfg["width"], cfg["height"])
    if args.tile_rows:                                     # one rank's share of an N-GPU run: tile rows first, first + stride, ...
        first, stride = (int(v) for v in args.tile_rows.split(","))
        r.SetTileRows(first, stride)
    batch = r.get_policy()["max_batch"]
    r.Accumulate(batch)
    c = r.counters()
    print(json.dumps({"batch": batch, "rays": c["rays"], "shadow_rays": c["shadow_rays"]}), flush=True)
    r.close()


def run_reaped(cmd, timeout, log, **kw):
    """subprocess.run for the helper processes of this script, each in a session of its own: when the direct child has ended (or run out
    of time) whatever else it started — rocprofv3 runs the program as a grandchild, and may leave helpers — is signalled through the
    process group and waited for, so nothing of ours is alive when bench.py ends (BENCH_r02: procs_at_end 1)."""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True, **kw)
    log(f"child pid {p.pid}: {' '.join(cmd[:3])} ...")
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        out, err = "", f"timed out after {timeout}s"
    finally:
        for sig in (signal.SIGTERM, signal.SIGKILL):       # the exact process group we created, nothing matched by name
            try:
                os.killpg(p.pid, sig)
            except (ProcessLookupError, PermissionError):
                break
            try:
                p.wait(timeout=5)
            except subprocess.TimeoutExpired:
                pass
            time.sleep(0.2)
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            pass
    return subprocess.CompletedProcess(cmd, p.returncode if p.returncode is not None else -9, out, err)


def run_pmc_pass(counters, args, log):
    """`rocprofv3 --pmc <counters> -- python3 bench.py --pmc-child`: returns ({kernel class: {counter: sum, 'launches', 'us'}}, child info) or None."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out_dir = tempfile.mkdtemp(prefix="mirt_pmc_", dir="/tmp")
    cmd = [exe, "--pmc", *counters.split(), "--output-format", "csv", "-d", out_dir, "--",
           sys.executable, os.path.abspath(__file__), "--pmc-child", "--config", args.config, "--max-batch", str(args.max_batch)]
    if getattr(args, "share", None):
        cmd += ["--tile-rows", args.share]
    try:
        p = run_reaped(cmd, 240, log, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"))
        info = None
        for line in p.stdout.splitlines():
            if line.startswith("{") and '"batch"' in line:
                info = json.loads(line)
        files = glob.glob(os.path.join(out_dir, "**", "*_counter_collection.csv"), recursive=True)
        if p.returncode != 0 or info is None or not files:
            log(f"pmc pass [{counters}] failed (rc {p.returncode}): {p.stderr[-300:]}")
            return None
        agg = {}
        for row in csv.DictReader(open(max(files, key=os.path.getmtime))):
            name = row["Kernel_Name"]
            if "mirt::k_trace_fat" in name or "mirt::" not in name:
                continue
            klass = "trace" if ("mirt::k_trace<" in name or "mirt::k_primary_" in name) else "shade" if "mirt::k_shade<" in name else "other"   # k_primary_*: Traverse of the camera rays
            a = agg.setdefault(klass, {"launches": set(), "us": 0.0})
            a[row["Counter_Name"]] = a.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
            if row["Dispatch_Id"] not in a["launches"]:
                a["launches"].add(row["Dispatch_Id"])
                a["us"] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        for a in agg.values():
            a["launches"] = len(a["launches"])
        return agg, info
    except Exception as e:                                 # the bench line must not depend on the profiler
        log(f"pmc pass [{counters}] skipped: {e}")
        return None
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def collect_pmc(args, log):
    t0 = time.perf_counter()
    out = {"command": "rocprofv3 --pmc <counters> --output-format csv -- python3 bench.py --pmc-child --config %s (one batch, one kernel at a time)" % args.config}
    sq = run_pmc_pass(SQ_COUNTERS, args, log)
    if sq is None:
        return None
    out["sq"], out["child"] = sq
    # TCC: FETCH_SIZE takes 3 of the 4 slots, WRITE_SIZE 2 -> separate passes; GRBM: the clock the chip held; then the VALU instruction mix
    passes = [("mix", MIX_COUNTERS), ("FETCH_SIZE", "FETCH_SIZE"), ("WRITE_SIZE", "WRITE_SIZE")]
    if not getattr(args, "share", None):                   # the clock and the L1 gather path: single-GPU runs only (the other ranks are waiting)
        passes += [("GRBM_GUI_ACTIVE", "GRBM_GUI_ACTIVE"), ("vmem", "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TA_TA_BUSY_sum GRBM_GUI_ACTIVE")]
    for name, counters in passes:
        r = run_pmc_pass(counters, args, log)
        out[name] = r[0] if r else None
    log(f"pmc passes took {time.perf_counter() - t0:.1f}s")
    return out


# ---- CPU baseline ------------------------------------------------------------------------------------------------
def cpu_baseline(mirt, cfg, log):
    """The reference's own CPU path as restated in oracle/ (the reference itself cannot be built here): stream-BVH traversal
    (BVH.hpp:320-358) with the AVX2 8-ray sphere kernel, tiles over the host threads of this job — on a BOUNDED sample: the same
    scene, camera and policy rendered at a reduced resolution (rays/s does not depend on the pixel count), at least 4 accumulations
    (SURVEY.md §8d), sized by a short probe to about 15 s of CPU work."""
    import oracle_binding as ob
    hw_threads = os.cpu_count() or 1
    threads = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else hw_threads, 16)   # the GPU box gives a 1-GPU job a 16-CPU share
    scene_fn = lambda: mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])   # noqa: E731
    o = ob.Oracle(scene_fn(), max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], trav_mode=ob.TRAV_STREAM_BVH, threads=threads)
    o.Resize(256, 256)
    t0 = time.perf_counter(); o.Accumulate(1); probe = max(time.perf_counter() - t0, 1e-3)          # seconds per accumulation of 65536 pixels
    side = 256
    for cand in (384, 512, 768, 1024):                      # the largest sample whose 4 accumulations stay below ~20 s
        if cand <= min(cfg["width"], cfg["height"]) and probe * (cand / 256.0) ** 2 * 4 <= 20.0:
            side = cand
    n = int(max(4, min(16, 15.0 / (probe * (side / 256.0) ** 2))))
    o.Resize(side, side)
    o.ResetAccumulator()
    r0 = o.counters()["rays"]
    t0 = time.perf_counter(); o.Accumulate(n); t1 = time.perf_counter() - t0
    rays = o.counters()["rays"] - r0
    log(f"cpu baseline: {n} accumulations at {side}x{side}, {rays} rays in {t1:.2f}s on {threads} of {hw_threads} hardware threads")
    out = {"value": rays / t1 / 1e6, "unit": "Mray/s", "cores": threads, "host_hardware_threads": hw_threads, "kind": "port",
           "sample": f"{n} accumulations of the same S({cfg['n']}) scene, camera and policy at {side}x{side} px (instead of {cfg['width']}x{cfg['height']}), oracle stream-BVH "
                     f"mode (reference BVH.hpp:320-358 restated; the reference itself is unbuildable here), {threads} threads = this job's share of the box's {hw_threads} hardware threads"}
    o.close()
    try:    # the reference AS SHIPPED traverses nothing (#define USEBVH false, BVH.hpp:307): brute force over all spheres (SURVEY.md §8d asks for both)
        b = ob.Oracle(scene_fn(), max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], trav_mode=ob.TRAV_BRUTE, threads=threads)
        b.Resize(32, 32)
        t0 = time.perf_counter(); b.Accumulate(1); probe = max(time.perf_counter() - t0, 1e-4)      # per accumulation of 1024 pixels
        win = 32
        for cand in (48, 64, 96, 128, 192, 256):
            if probe * (cand / 32.0) ** 2 * 4 <= 6.0:
                win = cand
        b.Resize(win, win); b.ResetAccumulator()
        r0 = b.counters()["rays"]
        t0 = time.perf_counter(); b.Accumulate(4); dtb = time.perf_counter() - t0
        out["as_shipped_brute_force"] = {"value": (b.counters()["rays"] - r0) / dtb / 1e6, "unit": "Mray/s", "cores": threads,
                                         "sample": f"4 accumulations at {win}x{win} px of the same scene and camera (USEBVH false: every ray tests all {cfg['n']} spheres)"}
        b.close()
    except Exception as e:
        log(f"brute-force cpu baseline skipped: {e}")
    return out


def dump_outputs(out_dir, acc, log):
    """--dump-outputs: `acc` = the whole image's accumulator as a torch tensor [tile][bucket][rgb][256] f32 (device or host)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    n_tiles = acc.shape[0]
    tile_bytes = acc[0].numel() * acc.element_size()
    n = min(n_tiles, DUMP_SAMPLE_TILES, DUMP_SAMPLE_BYTES // tile_bytes)
    idx = np.sort(np.random.default_rng(0).choice(n_tiles, n, replace=False))
    sample = acc[torch.from_numpy(idx).to(acc.device)].cpu().numpy()
    sums = torch.cat([acc[i:i + 4096].double().sum(dim=(1, 3)).cpu() for i in range(0, n_tiles, 4096)]).numpy()
    np.save(os.path.join(out_dir, "accumulator_tiles.npy"), np.ascontiguousarray(sample, dtype=np.float32))
    np.save(os.path.join(out_dir, "accumulator_tile_sums.npy"), np.ascontiguousarray(sums, dtype=np.float64))
    log(f"outputs: {n} of {n_tiles} accumulator tiles and {n_tiles} tile sums written to {out_dir}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="cfg4", choices=["cfg2", "cfg3", "cfg4", "cfg5"],
                    help="BASELINE config (default cfg4, the one the metric is quoted on). Every config keeps its own fixed image and splits its tile rows over the ranks")
    ap.add_argument("--spp", type=int, default=64, help="accumulations (Renderer::Accumulate() calls) per step")
    ap.add_argument("--streams", type=int, default=0, help="batches in flight on separate HIP streams (0 = library default, 3)")
    ap.add_argument("--max-batch", type=int, default=0, help="Accumulate() calls traced together as one batch (0 = library default: about 1 G primary rays, at most 256 calls)")
    ap.add_argument("--aux-steps", type=int, default=2, help="steps of the roofline passes (per-kernel HIP-event timing, counting replay)")
    ap.add_argument("--gpu-build", action="store_true", help="policy.gpu_build: the traversal tree from the GPU LBVH builder instead of the host SAH sweep (measurements)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-counts", action="store_true", help="skip the per-kernel timing and counting passes (roofline becomes null)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc child passes")
    ap.add_argument("--group", action="store_true", help="one process drives --gpus N devices through the library's mirt_group_* entry points (in-library RCCL gather) "
                    "instead of one process per GPU; MIRT_BENCH_DEVICES=0,0 names the devices explicitly (rehearsal with members sharing a device)")
    ap.add_argument("--no-group-host", action="store_true", help="N > 1 under torch.distributed.run: skip the child run of the --group host")
    ap.add_argument("--full", action="store_true", help="also run every secondary measurement: roofline / PMC passes, the tree-walking comparison, "
                    "the CPU baseline, the group host child for N > 1 (a plain run times the K steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="after the timed steps, write the accumulator they produced to DIR/*.npy")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tile-rows", default="", help=argparse.SUPPRESS)      # --pmc-child: "first,stride" = one rank's share of the image
    args = ap.parse_args()
    if args.pmc_child:
        return pmc_child(args)
    if args.group:
        return group_main(args)
    if not args.full:                                      # a plain run: set-up, warm-up, the K timed steps, the line
        args.no_counts = args.no_pmc = args.no_cpu_baseline = args.no_group_host = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch multi-GPU runs with torch.distributed.run (one process per GPU)")
        args.gpus = world

    def log(msg):
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    # PMC child passes first, on rank 0: nothing in this process has touched the GPU or joined the process group yet (the other ranks wait
    # in init_process_group).  For N > 1 the child renders rank 0's share of the image (tile rows 0, N, 2N, ...).
    pmc = None
    if rank == 0 and not args.no_pmc and not args.no_counts:
        args.share = f"0,{world}" if world > 1 else ""
        pmc = collect_pmc(args, log)

    import torch
    mirt = load_mirt()
    # Rehearsal knobs (single-GPU box): MIRT_BENCH_SHARE_GPU=1 puts every rank on cuda:0, MIRT_BENCH_BACKEND=gloo replaces RCCL
    # (which refuses two ranks on one device); the gather then stages through host memory.  Never set by the driver.
    backend = os.environ.get("MIRT_BENCH_BACKEND", "nccl")
    if os.environ.get("MIRT_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    comm_device = "cuda" if backend == "nccl" else "cpu"

    cfg = dict(mirt.scene.CONFIGS[args.config])
    width, height = cfg["width"], cfg["height"]
    h_tiles, v_tiles = width // 16, height // 16
    tiles = h_tiles * v_tiles
    first_row, row_stride, n_rows = mirt.distributed.tile_rows(v_tiles, rank, world)     # interleaved tile rows: every rank sees sky and ground alike
    count = n_rows * h_tiles

    r = make_renderer(mirt, cfg, local_rank, profile=False, streams=args.streams, max_batch=args.max_batch, gpu_build=args.gpu_build)
    r.Resize(width, height)
    if world > 1:
        r.SetTileRows(first_row, row_stride)
    spp, K, W = args.spp, args.steps, args.warmup
    batch, n_streams = r.get_policy()["max_batch"], r.get_policy()["streams"]     # the values in effect (0 = automatic: see batch planning in mirt_capi.hip)
    log(f"{args.config}: {width}x{height}, S({cfg['n']}), {spp} accumulations/step, batches of {batch} x {n_streams} in flight, {count} of {tiles} tiles on this rank")

    def sync_all():
        r.Synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # ---- timed pass: W warmup steps, then exactly K steps; no profiling, no counting ----
    for _ in range(W):
        r.Accumulate(spp)
    rays0 = r.counters()["rays"]
    sync_all()
    t0 = time.perf_counter()
    for _ in range(K):
        r.AccumulateAsync(spp)         # the K steps are bracketed by device synchronisation on both sides, not separated by it
    sync_all()
    elapsed = time.perf_counter() - t0
    rays_local = r.counters()["rays"] - rays0          # `rays` is counted by every launch (one atomic per kernel)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=comm_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        t = torch.tensor([float(rays_local)], dtype=torch.float64, device=comm_device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        rays_total = int(t.item())
    else:
        rays_total = rays_local

    # ---- one gather of the accumulated radiance to rank 0 (RCCL over xGMI), outside the timed region ----
    gather_ms = None
    if dist is not None:
        local = mirt.distributed.device_tensor(*r.accumulator_device(), shape=(count, cfg["buckets"], 3, 256))
        if comm_device == "cpu":
            local = local.cpu()
        sync_all()
        g0 = time.perf_counter()
        full = mirt.distributed.gather_accumulator_rows(local, h_tiles, v_tiles, rank, world, cfg["buckets"])
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - g0) * 1e3
        if rank == 0:
            assert tuple(full.shape) == (tiles, cfg["buckets"], 3, 256)
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, full, log)
        del full
    elif args.dump_outputs:
        dump_outputs(args.dump_outputs, mirt.distributed.device_tensor(*r.accumulator_device(), shape=(count, cfg["buckets"], 3, 256)), log)

    # ---- the same steps with every camera ray walking the tree by itself (policy.trace_primary_rays = 1), for comparison: by default the
    #      jittered samples of a pixel share one cone traversal per batch (kernels.hpp, k_primary_cand); results are bit-identical ----
    value_walk = None
    if not args.no_counts and world == 1:
        r.set_policy(trace_primary_rays=1)
        r.ResetAccumulator()
        for _ in range(W):
            r.Accumulate(spp)
        sync_all()
        c0 = r.counters()["rays"]; t1 = time.perf_counter()
        for _ in range(max(1, min(args.aux_steps, K))):
            r.AccumulateAsync(spp)
        sync_all()
        value_walk = (r.counters()["rays"] - c0) / (time.perf_counter() - t1) / 1e6
        r.set_policy(trace_primary_rays=0)

    # ---- roofline passes (rank 0's share of the image): the first `aux` steps after the warmup again, (a) with ONE batch in
    #      flight and HIP events around every launch, so a launch's duration is the kernel's own; (b) with the kernels counting
    #      the boxes and spheres they test ----
    ktimes, counts = None, None
    aux = max(1, min(args.aux_steps, K))
    if not args.no_counts:
        r.set_policy(streams=1, profile=1, count_traffic=0)
        r.ResetAccumulator()
        for _ in range(W):
            r.Accumulate(spp)
        r.kernel_times(reset=True)
        for _ in range(aux):
            r.Accumulate(spp)
        ktimes = r.kernel_times(reset=True)
        r.set_policy(count_traffic=1, profile=0)
        r.ResetAccumulator()
        for _ in range(W):
            r.Accumulate(spp)
        c0 = r.counters()
        for _ in range(aux):
            r.Accumulate(spp)
        c1 = r.counters()
        counts = {k: c1[k] - c0[k] for k in c1}

    if rank == 0:
        value = rays_total / elapsed / 1e6
        roofline = None
        if ktimes and counts and ktimes["trace"]["launches"]:
            tr, sh = ktimes["trace"], ktimes["shade"]
            trace_s = tr["ms"] * 1e-3
            traced = counts["rays"] + counts["shadow_rays"]
            ab = algorithmic_bytes(counts)
            roofline = {"bound": "valu", "kernel": "k_trace", "achieved": None, "peak": VALU_PEAK_GCYC, "unit": "G VALU-issuing SIMD-cycles/s", "frac": None, "traffic": None,
                        "peak_definition": "256 CUs x 4 SIMDs x 2.4 GHz max clock: a VALU instruction issuing on every SIMD in every quad-cycle with all 64 lanes at work; issue_achieved = 4 x (SQ_INSTS_VALU - "
                                           "SQ_ACTIVE_INST_VALU2) per second, achieved = issue_achieved x lane_utilisation; frac = useful_lane_frac (issue_frac: lanes not weighed; arithmetic_frac: box and "
                                           "sphere tests only, against the all-FMA rate); north_star's HBM roofline is the secondary `hbm` (a cache-resident tree is not HBM-bound)",
                        "launches": tr["launches"], "avg_launch_ms": tr["ms"] / tr["launches"],
                        "measured_with": f"HIP events on the launch stream, second live pass of {aux} step(s) with one batch in flight",
                        "traced_rays_per_launch": traced / tr["launches"],
                        "boxes_per_ray": counts["nodes"] / counts["rays"], "spheres_per_ray": counts["spheres"] / counts["rays"],
                        "boxes_per_shadow_ray": counts["shadow_nodes"] / max(counts["shadow_rays"], 1)}
            hbm = {"bound": "hbm", "achieved": ab / trace_s / 1e9, "peak": HBM_PEAK_GBPS, "peak_measured_copy": 6290.0, "unit": "GB/s", "frac": ab / trace_s / 1e9 / HBM_PEAK_GBPS,
                   "algorithmic_bytes_per_launch": ab / tr["launches"], "traffic": None,
                   "note": "SURVEY.md §8d prices every BVH child box and sphere tested at 32 B against HBM; k_trace serves them from the tree top it stages in LDS and from L2, "
                           "so this secondary figure may exceed 1: HBM does not bound the kernel. `traffic` = HBM bytes per launch from this run's FETCH_SIZE / WRITE_SIZE passes"}
            if pmc and pmc.get("sq") and "trace" in pmc["sq"]:
                q, ch = pmc["sq"]["trace"], pmc["child"]
                ch_traced = ch["rays"] + ch["shadow_rays"]
                valu_per_ray = q["SQ_INSTS_VALU"] / ch_traced
                mix = (pmc.get("mix") or {}).get("trace")
                busy_per_ray = ach = None
                if mix and mix.get("SQ_INSTS_VALU"):
                    # issue quad-cycles = instructions - the quad-cycles that held two of them; scaled to this pass's instruction count per ray
                    busy_per_ray = 4.0 * (1.0 - mix["SQ_ACTIVE_INST_VALU2"] / mix["SQ_INSTS_VALU"]) * valu_per_ray
                    ach = busy_per_ray * traced / trace_s / 1e9
                lane_ach = valu_per_ray * traced * 64.0 / trace_s / 1e12
                lane_util = q["SQ_THREAD_CYCLES_VALU"] / max(64.0 * q["SQ_ACTIVE_INST_VALU"], 1.0)
                issue_frac = (ach / VALU_PEAK_GCYC) if ach else None
                arith_ops = (OPS_PER_BOX * (counts["nodes"] + counts["shadow_nodes"]) + OPS_PER_SPHERE * counts["spheres"] + OPS_PER_SHADOW_SPHERE * counts["shadow_spheres"])
                roofline.update(achieved=(ach * lane_util) if ach else None, frac=(issue_frac * lane_util) if ach else None,
                                unit="G VALU-issuing SIMD-cycles/s, weighted by the share of lanes doing work in them",
                                useful_lane_frac=(issue_frac * lane_util) if ach else None, issue_frac=issue_frac, issue_achieved=ach,
                                arithmetic_frac=arith_ops / trace_s / 1e12 / VALU_PEAK_TLANE,
                                arithmetic={"achieved": arith_ops / trace_s / 1e12, "peak": VALU_PEAK_TLANE, "unit": "Tlane-op/s",
                                            "ops_per_box": OPS_PER_BOX, "ops_per_sphere": OPS_PER_SPHERE, "ops_per_shadow_sphere": OPS_PER_SHADOW_SPHERE,
                                            "note": "slab-test and sphere-test VALU lane-operations (static counts from the ISA listing x the kernels' own box / sphere counters) per second "
                                                    "of k_trace, against the all-FMA vector rate; everything else a traversal executes (fetch, decode, ordering, stack, refill) is overhead here"},
                                valu_issue_cycles_per_traced_ray=busy_per_ray, valu_wave_instructions_per_traced_ray=valu_per_ray,
                                simd_cycles_per_valu_instruction=(VALU_PEAK_GCYC * 1e9 * trace_s) / (valu_per_ray * traced),
                                instruction_mix=({k.replace("SQ_INSTS_VALU_", "").lower(): v / mix["SQ_INSTS_VALU"] for k, v in mix.items() if k.startswith("SQ_INSTS_VALU_")} if mix else None),
                                dual_issue_share=(2.0 * mix["SQ_ACTIVE_INST_VALU2"] / mix["SQ_INSTS_VALU"]) if mix else None,
                                salu_per_valu=q["SQ_INSTS_SALU"] / q["SQ_INSTS_VALU"],
                                lane_utilisation=lane_util,
                                wait_share=q["SQ_WAIT_ANY"] / max(q["SQ_WAVE_CYCLES"], 1.0),
                                lane_instructions={"achieved": lane_ach, "peak": VALU_PEAK_TLANE, "unit": "Tlane-inst/s", "frac": lane_ach / VALU_PEAK_TLANE,
                                                   "note": "against the all-FMA issue rate (one wave64 instruction per 2 cycles per SIMD = the 157.3 TFLOP/s vector peak / 2 flop); "
                                                           "k_trace's mix is ~80 % half-rate instructions (4 cycles), see profiles/r02/valu_rates.txt"},
                                pmc={"source": pmc["command"], "batch": ch["batch"], "launches": q["launches"], "k_trace_ms_under_pmc": q["us"] / 1e3,
                                     "traced_rays": ch_traced, "SQ_INSTS_VALU": q["SQ_INSTS_VALU"], "SQ_ACTIVE_INST_VALU2_per_inst": (mix["SQ_ACTIVE_INST_VALU2"] / mix["SQ_INSTS_VALU"]) if mix else None},
                                note="issue_achieved = VALU issue quad-cycles x 4 per traced ray (k_trace dispatches of one batch, this run's rocprofv3 --pmc child passes) x rays traced per "
                                     "second in the HIP-event pass; lane_utilisation = SQ_THREAD_CYCLES_VALU / (64 x SQ_ACTIVE_INST_VALU); frac = useful_lane_frac = issue_frac x lane_utilisation")
                gr = pmc.get("GRBM_GUI_ACTIVE")
                if gr and "trace" in gr and gr["trace"]["us"] > 0:
                    # MI355X_MICROARCH.md "DVFS give-back": effective clock = GRBM_GUI_ACTIVE (summed over the 8 XCDs) / 8 / kernel time
                    ghz = gr["trace"]["GRBM_GUI_ACTIVE"] / 8.0 / (gr["trace"]["us"] * 1e-6) / 1e9
                    roofline["clock_GHz_during_k_trace"] = ghz
                    roofline["issue_frac_at_that_clock"] = (ach / (256 * 4 * ghz)) if ach else None
                vm = (pmc.get("vmem") or {}).get("trace")
                if vm and vm.get("GRBM_GUI_ACTIVE"):
                    # the second unit k_trace leans on: every lane of a node / leaf pass gathers its own 32-B record or 16-B sphere, and a CU's
                    # L1 (TCP) takes about one cache-line access per cycle.  GRBM_GUI_ACTIVE is summed over the 8 XCDs -> CU-cycles = x 32.
                    cu_cycles = vm["GRBM_GUI_ACTIVE"] / 8.0 * 256.0
                    roofline["vector_memory"] = {"l1_line_accesses_per_cu_cycle": vm["TCP_TOTAL_CACHE_ACCESSES_sum"] / cu_cycles,
                                                 "l1_miss_share": vm["TCP_TCC_READ_REQ_sum"] / max(vm["TCP_TOTAL_CACHE_ACCESSES_sum"], 1.0),
                                                 "ta_busy_share": vm["TA_TA_BUSY_sum"] / cu_cycles,
                                                 "l1_line_accesses_per_traced_ray": vm["TCP_TOTAL_CACHE_ACCESSES_sum"] / ch_traced,
                                                 "note": "TCP_TOTAL_CACHE_ACCESSES_sum, TCP_TCC_READ_REQ_sum, TA_TA_BUSY_sum over the k_trace dispatches of the PMC child batch, "
                                                         "per CU-cycle (GRBM_GUI_ACTIVE / 8 x 256 CUs)"}
                f, w_ = pmc.get("FETCH_SIZE"), pmc.get("WRITE_SIZE")
                if f and w_ and "trace" in f and "trace" in w_:
                    # MI355X_MICROARCH.md §HBM: on gfx950 FETCH_SIZE reports half of the bytes of wide coalesced reads -> doubled; WRITE_SIZE is exact; both in KB
                    hbm["traffic"] = (2.0 * f["trace"]["FETCH_SIZE"] + w_["trace"]["WRITE_SIZE"]) * 1024.0 / f["trace"]["launches"]
                    hbm["traffic_fetch_bytes_x2"] = 2.0 * f["trace"]["FETCH_SIZE"] * 1024.0 / f["trace"]["launches"]
                    hbm["traffic_write_bytes"] = w_["trace"]["WRITE_SIZE"] * 1024.0 / w_["trace"]["launches"]
                    hbm["traffic_GBps"] = hbm["traffic"] / (q["us"] / q["launches"] * 1e-6) / 1e9
                    roofline["traffic"] = hbm["traffic"]
                    if "shade" in f and "shade" in w_:
                        roofline["shade_traffic"] = (2.0 * f["shade"]["FETCH_SIZE"] + w_["shade"]["WRITE_SIZE"]) * 1024.0 / f["shade"]["launches"]
            else:
                roofline["note"] = "rocprofv3 --pmc child pass unavailable: VALU instruction counts (achieved, frac) and HBM traffic not measured in this run"
            roofline["hbm"] = hbm
            if sh["launches"]:
                # second kernel: k_shade moves the ray streams and IS HBM-bound.  SURVEY.md §8d: 56 B read per ray shaded + 56 B written per
                # extension ray + 24 B of accumulator RMW per terminated path (bounce 0 has no stream here: its rays are generated in the kernels)
                primary = aux * spp * count * 256
                sb = 56.0 * (counts["rays"] - primary) + 56.0 * (counts["rays"] - primary) + 24.0 * counts["terminated"]
                roofline["shade"] = {"bound": "hbm", "kernel": "k_shade", "achieved": sb / (sh["ms"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                     "frac": sb / (sh["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, "launches": sh["launches"], "avg_launch_ms": sh["ms"] / sh["launches"],
                                     "traffic": roofline.pop("shade_traffic", None),
                                     "note": "§8d stream I/O of the extension rays only; the hit records it reads (8 B per ray) and the shadow-ray records it writes (32-68 B per NEE ray) are not in that figure"}
        out = {
            "metric": "Mray/s (primary+bounce)", "value": value, "unit": "Mray/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": (f"{args.config}: {width}x{height} px, S({cfg['n']}) spheres + SAH BVH, MIS, Policy.max_bounces={cfg['max_bounces']} "
                                    f"(primary+{cfg['max_bounces'] - 1} bounces), {cfg['buckets']} buckets, {spp} accumulations/step; fixed image, tile rows split over the GPUs"),
                       "image": f"{width}x{height}", "spp_per_step": spp, "spheres": cfg["n"], "max_bounces": cfg["max_bounces"], "buckets": cfg["buckets"],
                       "parallelism": f"tile rows interleaved over {world} GPUs, one RCCL gather" if world > 1 else "single GPU", "batches_in_flight": n_streams,
                       "accumulations_per_batch": min(batch, spp * K),     # the K steps are issued with mirt_accumulate_async: a batch may span steps
                       "accumulations_per_batch_limit": batch,
                       "primary_rays": "the jittered camera rays of a pixel share one cone traversal per batch that lists the spheres they can hit; every ray is then "
                                       "intersected with its pixel's list by the reference's arithmetic (policy.trace_primary_rays = 0, bit-identical results)"},
            "value_with_every_primary_ray_walking_the_tree": value_walk,
            "rays_per_step": rays_total / K,
            "shadow_rays_per_step": (counts["shadow_rays"] / aux) if counts else None,
            "kernel_ms_per_step": ({k: v["ms"] / aux for k, v in ktimes.items() if v["launches"]} if ktimes else None),
            "gather_ms": gather_ms,
            "roofline": roofline,
        }
        out["cpu_baseline"] = None if args.no_cpu_baseline else cpu_baseline(mirt, cfg, log)     # rank 0, outside every timed region (the other ranks wait below)
    r.close()                                              # every rank releases its GPU: streams, accumulator, scene
    if dist is not None:
        dist.barrier()
    # While rank 0 runs the group host over ALL the node's devices, the other ranks wait on the rendezvous store (host side): an RCCL barrier
    # would park a spinning kernel on every GPU the child is about to use.
    store = None
    if dist is not None and not args.no_group_host:
        try:
            store = dist.distributed_c10d._get_default_store()
        except Exception:
            store = None
    if rank == 0:
        if world > 1 and not args.no_group_host:
            out["group_host"] = group_host_child(args, world, log)
            if store is not None:
                store.set("mirt_group_host_done", "1")
        print(json.dumps(out), flush=True)
    elif store is not None:
        import datetime
        try:
            store.wait(["mirt_group_host_done"], datetime.timedelta(seconds=420))
        except Exception:
            pass
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def group_host_child(args, world, log):
    """N > 1: the library's own multi-GPU host (mirt_group_*: one process, ncclCommInitAll, grouped ncclSend / ncclRecv to the first device) on
    the same N devices, run once as a child process of rank 0 after every rank has released its GPU — so one driver command times the gather of
    both hosts.  A failure or a time-out of the child is reported, it never takes the bench line with it."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    if os.environ.get("MIRT_BENCH_SHARE_GPU") == "1":
        env["MIRT_BENCH_DEVICES"] = ",".join(["0"] * world)
    cmd = [sys.executable, os.path.abspath(__file__), "--group", "--gpus", str(world), "--steps", "1", "--warmup", "1", "--config", args.config, "--spp", str(args.spp),
           "--max-batch", str(args.max_batch), "--streams", str(args.streams)]
    p = run_reaped(cmd, 300, log, env=env)
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            return {k: d.get(k) for k in ("value", "unit", "ms_per_step", "gather_ms", "n_gpus", "steps", "warmup", "host", "devices")}
    return {"error": (p.stderr or "no output")[-400:], "returncode": p.returncode}


def group_main(args):
    """bench.py --group: the same workload through the library's group host — `Renderer<> renderer{scene}` as ONE object for the node
    (Application.cpp:514), one process driving every device, tile rows interleaved over them, the accumulator slabs gathered to the first
    device by the library itself (csrc/mirt_group.hip: ncclCommInitAll + a grouped ncclSend / ncclRecv per peer).  value = rays of all
    devices / wall time of the K steps; gather_ms = device time of the gather incl. the un-interleave."""
    def log(msg):
        print(f"[bench --group] {msg}", file=sys.stderr, flush=True)
    mirt = load_mirt()
    cfg = dict(mirt.scene.CONFIGS[args.config])
    devices = [int(v) for v in os.environ["MIRT_BENCH_DEVICES"].split(",")] if os.environ.get("MIRT_BENCH_DEVICES") else list(range(args.gpus))
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    g = mirt.GroupRenderer(sc, devices=devices, max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], mis=True, use_bvh=bool(cfg["use_bvh"]),
                           max_batch=args.max_batch, streams=args.streams)
    g.Resize(cfg["width"], cfg["height"])
    spp, K, W = args.spp, args.steps, args.warmup
    log(f"{args.config}: {cfg['width']}x{cfg['height']}, S({cfg['n']}), {spp} accumulations/step on devices {devices}")
    for _ in range(W):
        g.Accumulate(spp)
    rays0 = g.counters()["rays"]
    g.Synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        g.AccumulateAsync(spp)
    g.Synchronize()
    elapsed = time.perf_counter() - t0
    rays = g.counters()["rays"] - rays0
    g.Gather()                                             # the one exchange of the path, outside the timed region like the per-process host's
    gather_ms = g.gather_ms() if len(devices) > 1 else None
    if args.dump_outputs:
        import torch
        dump_outputs(args.dump_outputs, torch.from_numpy(g.accumulator()), log)
    out = {"metric": "Mray/s (primary+bounce)", "value": rays / elapsed / 1e6, "unit": "Mray/s", "n_gpus": len(devices), "steps": K, "warmup": W,
           "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "host": "group (one process, mirt_group_*)", "devices": devices,
           "config": {"workload": (f"{args.config}: {cfg['width']}x{cfg['height']} px, S({cfg['n']}) spheres + SAH BVH, MIS, Policy.max_bounces={cfg['max_bounces']}, "
                                   f"{cfg['buckets']} buckets, {spp} accumulations/step; fixed image, tile rows interleaved over the devices of one process"),
                      "image": f"{cfg['width']}x{cfg['height']}", "spp_per_step": spp, "spheres": cfg["n"], "max_bounces": cfg["max_bounces"], "buckets": cfg["buckets"],
                      "parallelism": f"mirt_group over {len(devices)} devices, in-library RCCL gather" if len(set(devices)) > 1 else f"mirt_group over {len(devices)} members sharing a device (rehearsal: device copies instead of RCCL)"},
           "rays_per_step": rays / K, "gather_ms": gather_ms, "roofline": None, "cpu_baseline": None}
    print(json.dumps(out), flush=True)
    g.close()


if __name__ == "__main__":
    main()
