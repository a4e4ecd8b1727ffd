#!/usr/bin/env python3
"""bench.py -- gridcell-region-timesteps/s of the weighted grid->region aggregation on MI355X.

A "step" is one pass of the hot path over one batch: out[T, R] = (X[T, G] . W[G, R]) / den[R].

Default workload (N=1) = BASELINE.json configs[1] in its dense north-star form ("c2-dense"):
T=365 daily steps, 0.25-degree grid G=720x1440=1,036,800, R=24,378 impact regions, fp32, W a
dense (gridcell x region) matrix generated on the device (101 GB, hash of (g, r, seed)); inputs
are resident in HBM before the timed region.  With --full the same run also times "c2-real" / "c3-real" (the
sparse segment-table form of configs[1] / [2]) and reports them under "secondary".

A plain run (no --full) does only what the headline needs: set up the workload, warm up, time exactly --steps steps,
write the outputs of the last timed step if --dump-outputs DIR is given, print the line.  Its `roofline` and
`cpu_baseline` are null.  --full adds everything else this script measures or checks: the secondary workloads, CPU
baselines, the dominant kernel's own timings and roofline, the boundary legs, and the N > 1 gather checks.

--dump-outputs DIR: DIR/out.npy holds what a caller of the timed path receives from its last timed step -- the (T, R)
block in the workload's dtype, on rank 0 of a sharded run the reassembled (T_job, R) series.  Above DUMP_LIMIT bytes
it is a fixed seeded sample of its rows.  The inputs depend only on the arguments, so two builds can be compared
output for output.

Workloads (--workload):
  c1          configs[0]: 2-degree grid, 100 regions, fp64 -- the reference's own CPU-sized case; the
              CPU oracle is timed on the FULL problem beside it
  c2-dense    configs[1], dense north-star form (default)
  c2-real     configs[1], segment-table form (HBM-bound)     c3-real  configs[2], fp64 + popwt
  c4          configs[3]: 10,950 daily steps, dense form, time axis cut over the ranks ("strong")
  c5-uniform  configs[4]: 50 x 365 rows, ~1 % non-zeros at uniformly random positions (entry-list form)
  c5-block    configs[4]: the block-local structure (tile-sparse MFMA form); c5-block-f64: the same in fp64
              (v_mfma_f64_16x16x4_f64)
For c4/c5 the rows of a run are shard_bounds(T_total, --shards)[rank]; --shards defaults to the
world size for c4 and to 8 for c5 (one rank's share of the 8-GPU job on a single GPU).

With --gpus N the time axis is sharded over N ranks (one process per GPU) and the region time series are
reassembled on rank 0 with an RCCL gather that overlaps the next step's compute; the default workload is weak
scaling (365 rows per rank).  The ranks may be started by torch.distributed.run (the driver's way: RANK /
LOCAL_RANK / WORLD_SIZE in the environment) or by this script itself: a plain `python bench.py --gpus N` starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child BEFORE anything touches the GPU,
relays rank 0's JSON line and returns the child's exit status (a rank whose LOCAL_RANK has no device exits
non-zero with a one-line reason).  --dry-run rehearses exactly that plumbing on CPU (gloo, no kernels).

The default N=1 run with --full carries every BASELINE config in its line: c2-dense is the headline; "secondary" holds c1,
c2-real, c3-real, one rank's share of c4 (1,369 rows on the c2-dense operand) and of c5 in both structures
(2,282 rows; block-local fp32, uniform fp32 and fp64), each with its own roofline and cpu_baseline.

Output (rank 0): ONE JSON line on stdout, below 6 KB -- the contract's keys, `roofline`, `cpu_baseline` and, with --full, one
short row per workload of the run (compact_line()) -- and the full record (every secondary in full, boundary legs, CPU
legs) as one `BENCH_DETAIL {...}` line on stderr; with --full also written to the files emit() names.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3    # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 flop/clk/CU
PEAK_F64_MFMA_TFLOPS = 78.6     # half the fp32 rate
PEAK_HBM_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
WORKLOADS = ["c1", "c2-dense", "c2-real", "c3-real", "c4", "c5-block", "c5-uniform", "c5-block-f64", "c5-uniform-f64"]
DENSE_FAMILY = ("c2-dense", "c4", "c5-block", "c5-uniform", "c5-block-f64", "c5-uniform-f64")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c2-dense", choices=WORKLOADS)
    ap.add_argument("--T", type=int, default=0, help="rows per rank (overrides the workload's own)")
    ap.add_argument("--shards", type=int, default=0, help="c4/c5: cut T_total into this many shards, this rank takes its own")
    ap.add_argument("--nlat", type=int, default=720)
    ap.add_argument("--nlon", type=int, default=1440)
    ap.add_argument("--R", type=int, default=24378)
    ap.add_argument("--ksplit", type=int, default=0)
    ap.add_argument("--land-frac", type=float, default=0.30, help="experiment knob for c2-real")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline (secondaries, CPU baselines, kernel timings and roofline, "
                         "boundary legs, N > 1 gather checks); --no-secondary, --no-cpu-baseline, --ref-budget-s, "
                         "--max-auto-steps and --budget-s tune it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/out.npy (a seeded row sample above 64 MB)")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--dry-run", action="store_true",
                    help="rehearse the launcher and the rank plumbing on CPU (gloo, no kernels, value 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--ref-budget-s", type=float, default=20.0,
                    help="seconds each reference-shaped CPU leg (NumPy scatter-add, pandas groupby) may take per workload")
    ap.add_argument("--max-auto-steps", type=int, default=0,
                    help="cap of the automatically sized timed regions of the secondaries (default 1000; profiler runs pass ~24: "
                         "a counter pass serialises every launch)")
    ap.add_argument("--warm-s", type=float, default=-1.0, help="seconds of warm-up before every timed region (default 0.3)")
    ap.add_argument("--budget-s", type=float, default=480.0,
                    help="wall-clock budget of the whole run: secondaries that would start beyond it are dropped with "
                         "\"skipped\": \"budget\" (the driver ends a run at 600 s)")
    ap.add_argument("--diag-lib", nargs="?", const="libwagg_diag.so", default=None, metavar="NAME",
                    help="load climate_toolbox_amd/lib/NAME (default libwagg_diag.so, `make diag`) instead of libwagg.so: "
                         "the build with the ablation knobs, or an experiment's variant; timing experiments only")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


def self_launch(a):
    """`python bench.py --gpus N` without torch.distributed.run in front: start the N ranks as a child job and relay
    rank 0's line.  Nothing here touches the GPU (no torch import, no libwagg call): the children are fresh
    processes, this one only waits."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for ln in proc.stdout:                 # the ranks' stderr passes straight through
        if ln.startswith("{"):
            line = ln
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if line is not None:
        sys.stdout.write(line)
        sys.stdout.flush()
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks exited cleanly without a JSON line\n")
        rc = 1
    return rc


def dry_run(a, rank, local_rank, world):
    """The rank plumbing without a GPU: gloo group, the shard rule, barrier + max-over-ranks timing, one line."""
    import torch
    import torch.distributed as dist
    from climate_toolbox_amd.timeshard import ShardedStep, shard_bounds
    ranks_seen = None
    if world > 1:
        dist.init_process_group("gloo")
        one = torch.ones(1)
        dist.all_reduce(one)                 # = world only if every rank took part (the N > 1 line's `rccl_ranks`, here over gloo)
        ranks_seen = int(round(float(one.item())))
    rows = [e - s0 for s0, e in shard_bounds(365 * world, world)]
    R = 16
    st = ShardedStep(lambda out: out.fill_(float(rank + 1)), lambda: torch.empty((rows[rank], R)), rows=rows, dst=0,
                     distributed=world > 1)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st.step()
    got = st.finish()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank == 0:
        ok = world == 1 or all(bool((got[sum(rows[:r]):sum(rows[:r + 1])] == r + 1).all()) for r in range(world))
        print(json.dumps({"metric": "gridcell-region-timesteps/sec", "value": 0.0, "unit": "gridcell-region-timesteps/s",
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / max(1, a.steps) * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "synthetic", "dry_run": True, "roofline": None, "cpu_baseline": None, "gather_ok": ok, "rccl_ranks": ranks_seen,
                          "backend": "gloo" if world > 1 else None,
                          "config": {"workload": "dry run: launcher + gloo gather only, no kernels", "T_job": sum(rows)}}),
              flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


COMPACT_LIMIT = 6144     # bytes: the driver parsed a 17 KB line in round 4 and failed on 28.5 KB in round 5; stay far below both
DUMP_LIMIT = 64 * 10**6  # bytes: --dump-outputs writes at most this much in all


def _sig(x, n=6):
    """floats to n significant digits (json size), everything else untouched"""
    if isinstance(x, float):
        return float("%.*g" % (n, x)) if x == x and x not in (float("inf"), float("-inf")) else None
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(line, limit=COMPACT_LIMIT):
    """The line that goes to STDOUT: the contract's keys, the dominant kernel's roofline, the CPU baseline and one short
    row per workload of the run -- under `limit` bytes whatever the run held.  Everything else (sorted samples, plan
    dumps, boundary legs, the secondaries' full entries) is the DETAIL: one `BENCH_DETAIL {...}` line on stderr and
    gpurun_out/bench_line_n<N>.json.  (Round 5's single 28.5 KB line was valid JSON and the driver still recorded
    `parsed: null`.)"""
    c = _pick(line, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "median_ms", "min_ms", "max_ms",
                     "higher_is_better", "scaling", "scaling_measured", "vs_baseline", "dtype", "data", "dry_run", "rehearsal"))
    c["config"] = _pick(line.get("config") or {}, ("workload", "T_per_gpu", "T_job", "G", "R", "parallelism", "nnz"))
    rf = line.get("roofline")
    c["roofline"] = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "frac_basis", "traffic", "traffic_source", "kernel",
                               "kernel_ms_median", "kernel_ms_min", "kernel_ms_max", "kernel_launches", "kernel_clock",
                               "event_overhead_ms", "frac_net",
                               "algorithmic_flops_per_launch", "algorithmic_bytes_per_launch", "achieved_on_traffic",
                               "frac_on_traffic")) if rf else None
    cb = line.get("cpu_baseline")
    c["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "wall_s", "sample")) if cb else None
    c.update(_pick(line, ("gather_ok", "rccl_ranks", "backend", "gather_ms", "gather_bytes", "per_rank_ms", "warmup_done",
                          "step_outlier", "elapsed_s", "plan_build_s")))
    if "cpu_reference_shaped_s" in line:
        c["cpu_reference_shaped_s"] = line["cpu_reference_shaped_s"]
    if line.get("summary"):
        c["summary"] = line["summary"]
    c["detail"] = "stderr line `BENCH_DETAIL {...}`; gpurun_out/bench_line_n%s.json" % line.get("n_gpus", 1)
    c = _sig(c)

    def size():
        return len(json.dumps(c, separators=(",", ":")))

    # a line that is still too long sheds what matters least, in this order -- never the contract's keys
    if size() > limit and isinstance(c.get("summary"), dict):
        c["summary"].pop("columns", None)
    if size() > limit:
        for d in (c, c["config"], c.get("roofline") or {}, c.get("cpu_baseline") or {}):
            for k, v in d.items():
                if isinstance(v, str) and len(v) > 120:
                    d[k] = v[:117] + "..."
    if size() > limit and isinstance(c.get("summary"), dict):
        c["summary"]["rows"] = [_pick(r, ("wl", "step_ms", "kernel_ms", "frac", "skipped")) for r in c["summary"]["rows"]]
    if size() > limit and isinstance(c.get("per_rank_ms"), list) and len(c["per_rank_ms"]) > 16:
        pr = c["per_rank_ms"]
        c["per_rank_ms"] = {"n": len(pr), "min": min(pr), "max": max(pr)}
    if size() > limit:
        c.pop("summary", None)
    return json.dumps(c, separators=(",", ":"))


def emit(line, world, detail_files=True):
    """rank 0: the detail to stderr, then the compact line -- the ONLY thing on stdout; with ``detail_files`` (--full)
    both records are also written to the files below."""
    full = json.dumps(line)
    text = compact_line(line)
    sys.stderr.write("BENCH_DETAIL " + full + "\n")
    sys.stderr.flush()
    print(text, flush=True)
    if not detail_files:
        return
    try:                                        # (gpurun merges gpurun_out/ back)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_line_n%d.json" % world), "w") as f:
            f.write(full + "\n")
        with open(os.path.join(ROOT, "gpurun_out", "bench_compact_n%d.json" % world), "w") as f:
            f.write(text + "\n")
    except OSError:
        pass


def load_traffic(workload):
    """(HBM bytes per launch, where that number comes from).  It is NOT measured by this run: it is
    the figure tools/summarize_prof.py derived from separate rocprofv3 --pmc passes and committed to
    profiles/traffic.json (PMC collection needs its own profiler runs, see profiles/README.md)."""
    p = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(p) as f:
            e = json.load(f).get(workload)
        if not e:
            return None, None
        return e.get("hbm_bytes_per_launch"), "profiles/traffic.json <- %s (%s)" % (e.get("source"), e.get("measured", "round 1"))
    except Exception:
        return None, None


# wagg_plan_info.kernel_form (when the library reports it): the dominant kernel of a segment-table apply
PLAN_KERNEL = {}


def sparse_algorithmic_bytes(T, G, R, nnz, b):
    # b*T*G + (b+4)*nnz + 4*(G+1) + b*T*R + b*R
    return b * T * G + (b + 4) * nnz + 4 * (G + 1) + b * T * R + b * R


WARM_S = 0.3          # every timed region starts after at least this much of the SAME apply (clocks, caches, allocators warm)
FILL_S = 0.5          # secondaries: as many timed steps as fill this, at least 10 (the profile ring holds 1024 kernel timings)
MAX_AUTO_STEPS = 1000


def _agree_max(torch, dist, n):
    """ranks must run the same number of steps (every step holds a collective): the largest count any of them wants"""
    if not (dist.is_available() and dist.is_initialized()):
        return int(n)
    t = torch.tensor([int(n)], dtype=torch.int64, device="cpu" if dist.get_backend() == "gloo" else "cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return int(t.item())


LAUNCHES_PER_APPLY = 0      # of the last timed_steps() run with a profile: dominant-kernel launches of one apply


def timed_steps(torch, dist, step, finish, steps, warmup, world, profile_reset=None, auto_steps=False, min_steps=10, profile_read=None):
    """(wall seconds of exactly `steps` steps between barrier + synchronize on both sides, max over ranks;
    per-step milliseconds from event pairs on the compute stream -- recorded without any synchronisation;
    the number of timed steps; the number of warm-up steps actually run).
    Warm-up = the `warmup` steps asked for, then more of the same until WARM_S seconds of this very apply have run (a
    two-step warm-up of a 9 ms apply after seconds of plan building times a device that is still waking up).
    ``auto_steps``: the timed steps are max(min_steps, what fills FILL_S) instead of `steps` (>= 10 repeats).
    ``profile_reset()`` is called right before the timed region, so the library's kernel timings cover exactly it."""
    world = world if not (dist.is_available() and dist.is_initialized()) else max(world, 2)   # forced-dist rehearsal
    import math
    t0 = time.perf_counter()
    n_warm = max(1, warmup) if auto_steps or warmup > 0 else 0
    for _ in range(n_warm):
        step()
    finish()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    est = el / max(1, n_warm)                       # seconds per step (an over-estimate while things are cold)
    if n_warm:
        # (every rank asks -- also one that has warmed up long enough by its own clock: the agreement is a collective)
        extra = _agree_max(torch, dist, min(4000, int(math.ceil(max(0.0, WARM_S - el) / max(est, 1e-6)))))
        t1 = time.perf_counter()
        for _ in range(extra):
            step()
        finish()
        torch.cuda.synchronize()
        if extra:
            est = (time.perf_counter() - t1) / extra
        n_warm += extra
    if auto_steps:
        steps = _agree_max(torch, dist, max(min_steps, min(MAX_AUTO_STEPS, int(math.ceil(FILL_S / max(est, 1e-6))))))
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    global LAUNCHES_PER_APPLY
    LAUNCHES_PER_APPLY = 0
    if profile_reset is not None:
        if profile_read is not None:
            # one more untimed step under the profile alone: how many launches of its dominant kernel does one apply make?
            # (a ragged batch makes two; the library's ring holds the first 1,024 launches of the timed region, so the
            #  count cannot always be had from len(ring) / steps afterwards)
            profile_reset()
            step()
            finish()
            torch.cuda.synchronize()
            LAUNCHES_PER_APPLY = len(profile_read())
            if world > 1:
                dist.barrier()
        profile_reset()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    # (no cyclic-garbage collection inside the timed region: a full collection walks every object of the process -- the
    #  c2-real table alone holds 800,000 label strings -- and takes tens of milliseconds wherever an allocation triggers it)
    import gc
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for a_, b_ in ev:
            a_.record()
            step()
            b_.record()
        finish()                               # every queued gather has completed
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        gc.enable()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, sorted(a_.elapsed_time(b_) for a_, b_ in ev), steps, n_warm


def _spread(sorted_ms, prefix):
    """median / min / max of a sorted list of milliseconds, the list itself when it is short (quantiles otherwise), and
    `outlier` when the slowest sample is more than 1.5 x the median."""
    n = len(sorted_ms)
    if n == 0:
        return {}
    med = sorted_ms[n // 2]
    d = {prefix + "median": med, prefix + "min": sorted_ms[0], prefix + "max": sorted_ms[-1]}
    if n <= 64:
        d[prefix + "sorted"] = [round(x, 4) for x in sorted_ms]
    else:
        d[prefix + "quantiles"] = {q: round(sorted_ms[min(n - 1, int(n * f))], 4) for q, f in
                                   (("p01", 0.01), ("p10", 0.10), ("p50", 0.50), ("p90", 0.90), ("p99", 0.99))}
    d[prefix + "outlier"] = bool(sorted_ms[-1] > 1.5 * med)
    return d


def step_stats(per_step_ms):
    """median / minimum / maximum of the per-step device times (SURVEY 8d's timing protocol asks for median and min)."""
    d = _spread(per_step_ms, "step_ms_")
    return {"median_ms": d.get("step_ms_median"), "min_ms": d.get("step_ms_min"), "max_ms": d.get("step_ms_max"),
            "step_outlier": d.get("step_ms_outlier"),
            **({"step_ms_sorted": d["step_ms_sorted"]} if "step_ms_sorted" in d else {"step_ms_quantiles": d.get("step_ms_quantiles")})}


KERNEL_CLOCK = ("hipExtLaunchKernel start/stop events (wagg_profile_read): the dispatch itself plus the event pair's own floor "
                "(event_overhead_ms, measured with an empty kernel); profiles/*kernel_stats.csv hold rocprofv3's dispatch durations")
EVENT_OVERHEAD_MS = None     # median of wagg_profile_event_overhead, measured once per run on the compute stream


def kernel_stats(kms, steps=0, per_apply_known=0):
    """The dominant kernel's own durations over the timed steps (hipExtLaunchKernel start / stop events: the dispatch
    itself, no host time): the roofline is priced on the MEDIAN; mean, min, max and the sorted list ride along, and
    `outlier` says when the slowest launch took more than 1.5 x the median.  (step_ms_max >> kernel_ms_max = a gap between
    launches, i.e. the host; kernel_ms_max >> kernel_ms_median = the device itself ran a launch slowly.)"""
    per_apply = 1
    if per_apply_known and per_apply_known > 1:
        per_apply = per_apply_known
    elif steps and len(kms) > steps and len(kms) % steps == 0:
        per_apply = len(kms) // steps
    if per_apply > 1:
        # an apply that launches its dominant kernel more than once (a ragged batch: full row blocks, then the remainder): the
        # launches of one step are added up (whole applies only: the ring may have filled up in the middle of one)
        kms = [sum(kms[i * per_apply:(i + 1) * per_apply]) for i in range(len(kms) // per_apply)]
    ks = sorted(kms)
    d = _spread(ks, "kernel_ms_")
    if kms:
        # WHERE in launch order the slowest sample sits (VERDICT r5 Weak #7b: is a +18 % maximum the first launch after the
        # warm-up -- cold caches / clocks -- or somewhere in the middle -- the device itself?)
        d["kernel_ms_first"] = round(kms[0], 4)
        d["kernel_ms_argmax"] = max(range(len(kms)), key=kms.__getitem__)
    d["kernel_launches_per_apply"] = per_apply
    d["kernel_clock"] = KERNEL_CLOCK
    if EVENT_OVERHEAD_MS is not None:
        # the same roofline with the measured floor of this clock taken off (the figure to hold against rocprofv3's dispatch
        # durations in profiles/); `frac` itself stays on the raw reading
        d["event_overhead_ms"] = round(EVENT_OVERHEAD_MS, 5)
        d["kernel_ms_median_net"] = max(d["kernel_ms_median"] - per_apply * EVENT_OVERHEAD_MS, 0.0)
    d["kernel_ms_avg"] = sum(ks) / max(1, len(ks))
    d["kernel_launches"] = len(ks)
    return d


# ---- CPU baselines (rank 0, N = 1 only; bounded samples; the oracle is the thing timed here) -------
def cpu_baseline_dense(T, G, R, seed_w, fill=1.0, blocklocal=False):
    """The oracle's dense restatement (oracle/wagg_oracle.c, kind "port") on a bounded window of
    the same workload: Tw rows x Gw cells x Rw regions, threads = OpenMP default."""
    import numpy as np
    from oracle import c_oracle
    Tw, Gw, Rw = min(T, 365), min(G, 32768), min(R, 8192)
    rng = np.random.default_rng(0)
    X = (280.0 + 30.0 * rng.standard_normal((Tw, Gw))).astype(np.float32)
    c_oracle.dense_synth_sparse(X[:8], 0, min(Gw, 256), R, 0, min(Rw, 256), seed_w, fill, blocklocal)     # warm
    t0 = time.perf_counter()
    c_oracle.dense_synth_sparse(X, 0, Gw, R, 0, Rw, seed_w, fill, blocklocal)
    dt = time.perf_counter() - t0
    return {"value": Tw * Gw * Rw / dt, "unit": "gridcell-region-timesteps/s", "cores": c_oracle.threads(),
            "kind": "port", "wall_s": round(dt, 3),
            "sample": "oracle/wagg_oracle.c dense (fp64 accumulate, OpenMP; weights regenerated from the hashes, "
                      "fill=%g%s) on %d rows x %d cells x %d regions of this workload's operands"
                      % (fill, ", block-local" if blocklocal else "", Tw, Gw, Rw)}


try:
    AFFINITY_AT_START = os.sched_getaffinity(0)
except (AttributeError, OSError):
    AFFINITY_AT_START = None


def usable_cpus():
    """(threads worth starting, what limits them): the smallest of the logical CPUs, the affinity mask and the cgroup's CPU
    quota (v2 cpu.max / v1 cpu.cfs_quota_us), the physical cores when nothing else binds (2 hardware threads per core)."""
    n = os.cpu_count() or 1
    why = "os.cpu_count"
    try:
        aff = len(os.sched_getaffinity(0))
        if aff < n:
            n, why = aff, "affinity mask"
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = float(f.read()), float(g.read())
                if q > 0:
                    quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None and quota < n:
        n, why = max(1, int(quota)), "cgroup cpu quota (%.4g CPUs of %d visible)" % (quota, os.cpu_count() or 1)
    else:
        try:                                           # one thread per physical core (OMP_PLACES=cores)
            cpus = sorted(os.sched_getaffinity(0))
            cores = set()
            for c in cpus:
                base = "/sys/devices/system/cpu/cpu%d/topology/" % c
                with open(base + "physical_package_id") as f, open(base + "core_id") as g:
                    cores.add((f.read().strip(), g.read().strip()))
            if 0 < len(cores) < n:
                n, why = len(cores), "physical cores"
        except (AttributeError, OSError):
            pass
    return n, why


def cpu_baseline_sparse(X_host, cell, codes, w_eff, R, G, what):
    """The oracle's faithful single-threaded restatement (gather -> fp64 multiply -> group-sum ->
    divide, like the reference) on the sample handed in (the FULL workload for the segment-table
    configs: it is only ~0.4 s of CPU work), median and minimum of up to 15 repeats inside ~10 s; plus the
    best-effort CPU leg SURVEY 8d asks for -- the same sums with the timesteps dealt to all host cores
    (OpenMP, oracle/wagg_oracle.c::wagg_oracle_segments_omp_*; threads pinned one per core by OMP_PROC_BIND=spread
    OMP_PLACES=cores, which main() sets before anything loads an OpenMP runtime; result buffer allocated and touched once;
    3 warm calls, then 15 timed: median, min and the thread count) -- and scipy's CSC SpMM (one thread) for reference."""
    import numpy as np
    import scipy.sparse as sp
    from oracle import c_oracle
    Ts = X_host.shape[0]
    c_oracle.segments(X_host[:1], cell, codes, w_eff, R)

    def timed(fn, budget_s=10.0, max_reps=15, warm=0):
        for _ in range(warm):
            fn()
        ts, t_start = [], time.perf_counter()
        while len(ts) < max_reps and (len(ts) < 3 or time.perf_counter() - t_start < budget_s):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            if time.perf_counter() - t_start > budget_s and len(ts) >= 1:
                break
        ts.sort()
        return ts[len(ts) // 2], ts[0], len(ts)

    dt, dmin, reps = timed(lambda: c_oracle.segments(X_host, cell, codes, w_eff, R))
    buf = np.zeros((Ts, R), dtype=np.float64)                       # (touched: its pages exist before the first timed call)
    dto, domin, repso = timed(lambda: c_oracle.segments(X_host, cell, codes, w_eff, R, threaded=True, out=buf), warm=3)
    del buf
    keep = (codes >= 0) & ~np.isnan(w_eff)
    W = sp.coo_matrix((w_eff[keep], (cell[keep], codes[keep])), shape=(G, R)).tocsc()
    den = np.asarray(W.sum(axis=0)).ravel()

    def scipy_leg():
        Xs = np.nan_to_num(X_host.astype(np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (W.T @ Xs.T).T / den[None, :]

    dtb, dbmin, repsb = timed(scipy_leg, budget_s=5.0, max_reps=5)
    return {"value": Ts * G * R / dt, "unit": "gridcell-region-timesteps/s", "cores": 1, "kind": "port",
            "wall_s": round(dt, 4), "wall_s_min": round(dmin, 4), "repeats": reps, "nnz_timesteps_per_s": Ts * len(cell) / dt,
            "sample": "oracle/wagg_oracle.c segments_%s (single thread, like the reference), %s"
                      % ("f32" if X_host.dtype == np.float32 else "f64", what),
            "cpu_best": {"value": Ts * G * R / dto, "wall_s": round(dto, 5), "wall_s_min": round(domin, 5), "cores": c_oracle.threads(),
                         "repeats": repso, "warm_calls": 3, "kind": "port",
                         "omp": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OMP_PROC_BIND", "OMP_PLACES", "OMP_DYNAMIC")},
                         "threads_limited_by": usable_cpus()[1], "host_logical_cpus": os.cpu_count(),
                         "what": "the same C restatement with the timesteps dealt to every host core (OpenMP, one warm team, threads "
                                 "bound to cores, result buffer reused), same sample"},
            "cpu_scipy": {"value": Ts * G * R / dtb, "wall_s": round(dtb, 4), "wall_s_min": round(dbmin, 4), "cores": 1, "repeats": repsb,
                          "what": "scipy.sparse CSC^T @ X^T in fp64 (one thread), same sample"}}


def cpu_reference_shaped(X_host, lat, lon, df, wname, lev, budget_s=20.0):
    """What a caller of the REFERENCE pays on the host, in the reference's own shape (VERDICT r5 Missing #3): the literal
    NumPy restatement of aggregations.py:24-27 (label lookup + fancy-index gather of every segment row), :73 (backup
    fill), :78-80 (fp64 product temporary -> grouped sums -> division) -- oracle/ref_numpy.py::agg_scatter (np.add.at) and
    ::agg_pandas (DataFrame.groupby().sum()) -- single thread, on the same operands the C port above is timed on.
    Per leg: one call on ONE row (= the per-call fixed cost: label lookup, label factorisation), then 1 warm + 3 timed
    calls on as many leading rows as keep the leg inside `budget_s`; when that is fewer than all rows, the full-size
    figure is fixed + (timed - fixed) x T / rows and says so.  (xarray itself is not installed: this is the arithmetic
    the reference hands to NumPy / pandas, without xarray's own overheads -- a floor for the reference, not a ceiling.)"""
    import numpy as np
    from oracle import ref_numpy as O
    T = X_host.shape[0]
    nlat, nlon = len(lat), len(lon)
    seg = (df["lat"].values, df["lon"].values, df[wname].values, df["areawt"].values, df[lev].values)

    def call(fn, rows):
        t0 = time.perf_counter()
        fn(X_host[:rows].reshape(rows, nlat, nlon), ("time", "lat", "lon"), lat, lon, *seg)
        return time.perf_counter() - t0

    out = {"threads": 1, "what": "oracle/ref_numpy.py agg_scatter (gather -> fp64 product -> np.add.at) and agg_pandas "
                                 "(groupby().sum()): aggregations.py:24-27,73,78-80 restated literally, same operands as the C port"}
    for name, fn in (("numpy_scatter", O.agg_scatter), ("pandas_groupby", O.agg_pandas)):
        fixed = call(fn, 1)
        probe_rows = min(T, 8)
        probe = call(fn, probe_rows)
        per_row = max((probe - fixed) / max(1, probe_rows - 1), 1e-7)
        per_call = budget_s / 4.0                                     # 1 warm + 3 timed
        rows = T if fixed + T * per_row <= per_call else int(max(probe_rows, min(T, (per_call - fixed) / per_row)))
        call(fn, rows)
        ts = sorted(call(fn, rows) for _ in range(3))
        med = ts[1]
        fixed = min(fixed, med)                                       # (one noisy first call must not push the scaling below zero)
        full = med if rows == T else fixed + (med - fixed) * T / rows
        out[name] = {"wall_s": round(full, 4), "rows_timed": rows, "rows": T, "timed_wall_s": round(med, 4), "timed_min_s": round(ts[0], 4),
                     "fixed_s": round(fixed, 4), "scaled": rows != T, "value": T * nlat * nlon * len(set(seg[4].tolist())) / full}
    return out


def main():
    t_start = time.perf_counter()
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(a)              # before anything that could initialise the GPU
    global MAX_AUTO_STEPS, WARM_S
    if a.max_auto_steps > 0:
        MAX_AUTO_STEPS = a.max_auto_steps
    if a.warm_s >= 0:
        WARM_S = a.warm_s
    # the CPU legs' OpenMP team: one thread per core, bound, no dynamic adjustment -- set before ANY OpenMP runtime loads
    # (torch brings one; the oracle links another): a team placed by chance gave medians 6x their minimum in round 4
    os.environ.setdefault("OMP_PROC_BIND", "spread")
    os.environ.setdefault("OMP_PLACES", "cores")
    os.environ.setdefault("OMP_DYNAMIC", "false")
    # ... and no more threads than the CPU time this process may use: the GPU box shows 256 logical CPUs but its cgroup grants
    # 16 CPUs' worth of time (cpu.max = "1600000 100000"); 128 threads on that are throttled by the scheduler -- the round-4
    # line's all-cores leg had a median 6x its minimum for exactly that reason
    os.environ.setdefault("OMP_NUM_THREADS", str(usable_cpus()[0]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if a.dry_run:
        return dry_run(a, rank, local_rank, world)
    import numpy as np
    import torch
    import torch.distributed as dist
    n_dev = torch.cuda.device_count()      # (counting devices does not initialise the GPU)
    # WAGG_BENCH_REHEARSE=gloo: the N > 1 CONTROL FLOW of this script (strong splits, secondaries, ragged gathers, the line)
    # on a box with fewer GPUs than ranks: every rank computes on device 0, the blocks travel through host buffers over gloo.
    # Not a measurement -- the line says so -- and RCCL is not involved (tests/test_gpu_round4.py covers RCCL with one rank).
    rehearse = os.environ.get("WAGG_BENCH_REHEARSE") == "gloo" and world > 1
    if rehearse:
        local_rank = 0
    if local_rank >= n_dev:
        raise SystemExit("bench.py: rank %d (LOCAL_RANK %d) has no device: this box has %d GPU(s), --gpus %d"
                         % (rank, local_rank, n_dev, a.gpus))
    torch.cuda.set_device(local_rank)
    # WAGG_BENCH_FORCE_DIST=1 exercises the RCCL init + gather code path with a single rank (rehearsal
    # on a one-GPU box); the timed step then includes the (trivial) gather exactly like N > 1 runs
    force_dist = os.environ.get("WAGG_BENCH_FORCE_DIST") == "1"
    use_dist = world > 1 or force_dist
    if use_dist:
        # stdout carries exactly one line (the JSON below): keep RCCL's version banner off it
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            os.environ.pop("NCCL_DEBUG")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    # proof that the collective backend saw every rank: an all-reduce of ones on device tensors (= N only if all took part)
    rccl_ranks = None
    if use_dist and a.full:
        one = torch.ones(1, dtype=torch.float32, device="cpu" if rehearse else "cuda")
        dist.all_reduce(one)
        rccl_ranks = int(round(float(one.item())))

    def out_of_budget():
        """a rank-consistent answer to "has the run used up --budget-s?" (every rank skips, or none: the steps hold collectives)"""
        over = 1 if time.perf_counter() - t_start > a.budget_s else 0
        if use_dist:
            t = torch.tensor([over], dtype=torch.int32, device="cpu" if rehearse else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            over = int(t.item())
        return bool(over)

    from climate_toolbox_amd import _lib, engine, synth
    if a.diag_lib:
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.path.basename(a.diag_lib))
    from climate_toolbox_amd.timeshard import ShardedStep, shard_bounds

    global EVENT_OVERHEAD_MS
    if a.full:
        try:
            EVENT_OVERHEAD_MS = engine.profile_event_overhead(128)[0]
        except Exception as e:                               # a diagnostic library without the symbol: the line says so
            sys.stderr.write("bench.py: no event-overhead measurement (%s)\n" % e)
    G, R = a.nlat * a.nlon, a.R
    scaling = "weak"
    C5_TOTAL, C4_TOTAL = 50 * 365, 10950

    def rows_for(wl, share=False):
        """(rows of this rank, rows of every rank, scaling) of a workload in this run; ``share``: one rank's share of
        the 8-GPU job (the secondary entries of the default N = 1 run)."""
        if wl in ("c4",) or wl.startswith("c5"):
            T_total = C4_TOTAL if wl == "c4" else C5_TOTAL
            shards = a.shards or (8 if share else (world if wl == "c4" or world > 1 else 8))
            bounds = shard_bounds(T_total, max(shards, world))
            rows_all = [e - s0 for s0, e in bounds][:world]
            if a.T:
                rows_all = [a.T] * world
            return rows_all[rank], rows_all, ("strong" if shards == world and not a.T else "weak")
        Tn = a.T or 365
        return Tn, [Tn] * world, "weak"

    def stepper(apply_fn, Tn, rows_all, Rr, dtype):
        if rehearse:                         # gloo moves host memory: compute into a device block, hand a host copy to the gather
            dev_block = torch.empty((Tn, Rr), dtype=dtype, device="cuda")

            def apply_to_host(out_host):
                apply_fn(dev_block)
                out_host.copy_(dev_block)
            return ShardedStep(apply_to_host, lambda: torch.empty((Tn, Rr), dtype=dtype), rows=rows_all, dst=0, distributed=True)
        return ShardedStep(apply_fn, lambda: torch.empty((Tn, Rr), dtype=dtype, device="cuda"), rows=rows_all, dst=0,
                           distributed=use_dist)

    outputs = {}                         # --dump-outputs: name -> host array

    def keep_output(st):
        """What a caller of the timed path receives from its last step -- this rank's block, on a sharded run the
        reassembled series (rank 0 only) -- as a host array; above DUMP_LIMIT bytes a fixed seeded sample of its rows."""
        out = st.finish() if st.distributed else st.bufs[(st.k - 1) & 1]
        if out is None:                  # (not the gather's destination)
            return
        row_bytes = out[0].numel() * out.element_size()
        if out.shape[0] * row_bytes > DUMP_LIMIT:
            keep = np.sort(np.random.default_rng(0).choice(out.shape[0], max(1, DUMP_LIMIT // row_bytes), replace=False))
            out = out[torch.from_numpy(keep).to(out.device)]
        outputs["out"] = out.cpu().numpy()

    def gather_check(st, Tn):
        """rank 0, distributed runs: the reassembled series holds this rank's last block in this rank's rows (the other
        ranks' rows are theirs to vouch for: the CPU gloo tests compare every block)."""
        if not (use_dist and a.full) or rank != 0:
            return None
        got = st.finish()
        return bool(got is not None and got.shape[0] == sum(st.rows) and torch.equal(got[:Tn], st.bufs[(st.k - 1) & 1]))

    def gather_timing(st, Tn, per_step_sorted):
        """N > 1 lines: what the driver needs to check the collective -- `gather_ms`: one BLOCKING gather of the real block
        (event pair / wall clock around timeshard.gather_time_shards, max over ranks); `per_rank_ms`: every rank's median
        step (all-gathered), so a straggler shows; `rccl_ranks`: the all-reduce proof from start-up."""
        if not (use_dist and a.full):
            return {}
        from climate_toolbox_amd.timeshard import gather_time_shards
        block = st.bufs[(st.k - 1) & 1]
        dev = "cpu" if rehearse else "cuda"
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        gather_time_shards(block, dst=0, rows=st.rows, out=st.gathered)
        if not rehearse:
            torch.cuda.synchronize()
        g_ms = (time.perf_counter() - t0) * 1e3
        t = torch.tensor([g_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        med = torch.tensor([per_step_sorted[len(per_step_sorted) // 2]], dtype=torch.float64, device=dev)
        allm = [torch.zeros_like(med) for _ in range(dist.get_world_size())]
        dist.all_gather(allm, med)
        return {"rccl_ranks": rccl_ranks, "backend": dist.get_backend(), "gather_ms": float(t.item()),
                "gather_bytes": int(sum(st.rows) * block.shape[1] * block.element_size()),
                "per_rank_ms": [round(float(x.item()), 4) for x in allm]}

    def on_traffic(roof, kavg, peak_gbs=PEAK_HBM_GBS):
        """The same roofline priced on the bytes the counters saw move (profiles/traffic.json), next to the
        algorithmic figure: a kernel that skips cells it does not need shows the difference here."""
        if roof.get("traffic"):
            roof["achieved_on_traffic"] = roof["traffic"] / kavg / 1e9
            roof["frac_on_traffic"] = roof["achieved_on_traffic"] / peak_gbs
            if roof["traffic"] < roof.get("algorithmic_bytes_per_launch", 0):
                roof["note"] = ("`achieved`/`frac` price SURVEY 8d's algorithmic bytes (all of X once); this kernel reads only "
                                "the 128-byte lines that hold referenced cells, so the fraction on those bytes can exceed 1: "
                                "`frac_on_traffic` is the one that says how close to the HBM the kernel runs")
        return roof

    def boundary_legs(Xs, lat, lon, df, plan, T, Gs, Rr):
        """What the kernel numbers leave out, on c2-real: the PCIe-inclusive rate of a host-resident
        field, the reference-named function end to end (device- and host-resident variable, cached plan), and the country
        level of the same table (agglev = "ISO": the other level the reference's docstring names, aggregations.py:104-106)."""
        from climate_toolbox_amd import _lib as L_, aggregations as A, minixr, weighted_aggregate_grid_to_regions
        out = {}
        # (the CPU legs ran OpenMP with OMP_PROC_BIND: the runtime bound THIS thread to one core when it entered its first
        #  parallel region, and threads started from here would inherit that mask -- the packing threads of the lines-only
        #  host path among them.  Back to the mask the process started with.)
        try:
            os.sched_setaffinity(0, AFFINITY_AT_START)
        except (AttributeError, OSError, TypeError):
            pass
        Xh = Xs.cpu().numpy()
        # (warm-up by time: staging pieces, the registration path, and -- measured -- host cores and copy engines that take
        #  several calls to leave their idle states: 25 GB/s for the first four calls of a run, 49 GB/s from then on)
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.5:
            plan.apply_host(Xh, flags=L_.HOST_PIN)
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            plan.apply_host(Xh, flags=L_.HOST_PIN)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        mid = ts[len(ts) // 2]
        out["host_resident"] = {"ms_per_step": mid * 1e3, "min_ms": ts[0] * 1e3, "max_ms": ts[-1] * 1e3, "calls": len(ts), "h2d_gbs": Xh.nbytes / mid / 1e9,
                                "what": "wagg_apply_host_ex_f32(WAGG_HOST_PIN) (row-block pipeline, arrays page-locked in place): every byte of X "
                                        "from host memory over PCIe, result back to host memory; PCIe-bound, never the headline value"}
        # the same with WAGG_HOST_LINES (what wagg_apply_host_f32 and the drop-in do by default): host threads pack the 128-byte
        # lines the table references into page-locked pieces, only those cross PCIe
        L_.host_stats(reset=True)
        tl = []
        for _ in range(9):
            t0 = time.perf_counter()
            plan.apply_host(Xh, flags=L_.HOST_PIN | L_.HOST_LINES)
            tl.append(time.perf_counter() - t0)
        st = L_.host_stats()
        tl = sorted(tl[2:])
        out["host_resident"]["lines_only"] = {"ms_per_step": tl[len(tl) // 2] * 1e3, "min_ms": tl[0] * 1e3, "max_ms": tl[-1] * 1e3, "calls": len(tl),
                                              "packed_fraction_of_x": st["lines_h2d_bytes"] / 9 / Xh.nbytes,
                                              "x_equivalent_gbs": Xh.nbytes / tl[len(tl) // 2] / 1e9,
                                              "wait_for_copy_engine_ms": st["lines_wait_copy_us"] / 9e3, "wait_for_packing_threads_ms": st["lines_wait_pack_us"] / 9e3,
                                              "blocks_retired_by_the_rate_watch": st["blocks_retired"],
                                              "packing_threads": min(12, max(usable_cpus()[0] // 2, usable_cpus()[0] - 4, 1))}
        # (round 6: the default packs only the quads that hold a referenced cell; the round-5 form -- whole 128-byte lines -- beside it)
        tw = []
        L_.host_stats(reset=True)
        for _ in range(7):
            t0 = time.perf_counter()
            plan.apply_host(Xh, flags=L_.HOST_PIN | L_.HOST_LINES | L_.HOST_LINES_WHOLE)
            tw.append(time.perf_counter() - t0)
        stw = L_.host_stats()
        tw = sorted(tw[2:])
        out["host_resident"]["lines_only"]["whole_128B_lines"] = {"ms_per_step": tw[len(tw) // 2] * 1e3, "min_ms": tw[0] * 1e3,
                                                                  "packed_fraction_of_x": stw["lines_h2d_bytes"] / 7 / Xh.nbytes}
        # the transforms the reference's callers run before they aggregate, on the same host-resident field (round 5): the fused
        # powers (tas_poly 1..4, transformations.py:188) and one set of Snyder degree days (tasmin = the field, tasmax = field + 9 K;
        # transformations.py:7-93) through the same pipeline, lines only; results (4 planes / 1 plane) back in host memory

        def med_ms(fn, n=5):
            fn()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return sorted(ts)[len(ts) // 2]

        both = L_.HOST_PIN | L_.HOST_LINES
        out["host_resident"]["tas_poly_1to4_lines_only_ms"] = med_ms(lambda: plan.apply_poly_host(Xh, -273.15, 4, flags=both))
        Xh_max = Xh + np.float32(9.0)
        out["host_resident"]["snyder_edd_lines_only_ms"] = med_ms(lambda: plan.apply_edd_host(Xh, Xh_max, [303.15], flags=both))
        del Xh_max

        def calls(ds, n=30, warm=15):
            # (15 warm-up calls: the first dozen calls after an idle spell run 2-3x slower on this platform whatever they do --
            #  host cores and the copy engines come out of their idle states; tools/dropin_split_timing.py shows the switch)
            for _ in range(warm):
                weighted_aggregate_grid_to_regions(ds, "tas", "areawt", "hierid", df)
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                weighted_aggregate_grid_to_regions(ds, "tas", "areawt", "hierid", df)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "calls": n}

        shape = (T, len(lat), len(lon))
        A._PLAN_CACHE.clear()
        dsd = minixr.Dataset({"tas": (("time", "lat", "lon"), Xs.reshape(shape))}, coords={"lat": lat, "lon": lon})
        dsh = minixr.Dataset({"tas": (("time", "lat", "lon"), Xh.reshape(shape))}, coords={"lat": lat, "lon": lon})
        from climate_toolbox_amd import prepare_weights
        df_plain = df
        prep = prepare_weights(df, "areawt", "hierid", lat=lat, lon=lon)
        d_dev, d_host = calls(dsd), calls(dsh, n=10, warm=5)
        df = prep                                                  # (calls() reads `df` of this scope)
        p_dev = calls(dsd)
        from climate_toolbox_amd import results_on_device
        with results_on_device():                                  # the result stays a CUDA tensor: no D2H copy, no wait
            r_dev = calls(dsd)
        df = df_plain
        out["dropin_ms"] = {"device_resident": d_dev, "host_resident": d_host, "device_resident_prepared_weights": p_dev,
                            "device_resident_device_result": r_dev,
                            "what": "weighted_aggregate_grid_to_regions(ds, 'tas', 'areawt', 'hierid', df) end to end (aggregations.py:87), "
                                    "cached plan, result returned as a host array; c2-real table (%d rows) as a DataFrame (fingerprinted "
                                    "by content on every call) and as prepare_weights(df, ...) (coded once); "
                                    "device_resident_device_result: prepared weights inside `with results_on_device():` -- the "
                                    "returned variable is a torch CUDA tensor" % len(df_plain)}
        A._PLAN_CACHE.clear()
        del dsd, dsh, Xh
        cell, codes, w_eff, uniq = synth.code_segments(df, lat, lon, "areawt", "ISO")
        t0 = time.perf_counter()
        iso = engine.SparsePlan(cell, codes, w_eff, Gs, len(uniq), row_len=len(lon))
        tb = time.perf_counter() - t0
        o = torch.empty((T, len(uniq)), dtype=Xs.dtype, device="cuda")
        for _ in range(3):
            iso.apply(Xs, out=o)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            iso.apply(Xs, out=o)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 20 * 1e3
        out["agglev_ISO"] = {"R": len(uniq), "ms_per_step": ms, "value": T * Gs * len(uniq) / (ms * 1e-3),
                             "unit": "gridcell-region-timesteps/s", "plan_build_s": round(tb, 4), "n_giant": int(iso.info["n_giant"]),
                             "what": "the same segment table aggregated to the country level (regions of thousands of cells each)"}
        iso.close()
        return out

    def net_of_events(roof, work, peak):
        """`frac_net`: the fraction on the median kernel time minus the event pair's floor (see KERNEL_CLOCK)"""
        net = roof.get("kernel_ms_median_net")
        if net:
            roof["frac_net"] = work / (net * 1e-3) / peak
        return roof

    def profile_reset():
        engine.profile_enable(True)       # (resets the ring: the timings read afterwards are those of the timed steps only)

    def run_sparse(dtype, small=False, steps=None, warmup=None, auto=False, keep_out=False):
        steps, warmup = steps or a.steps, a.warmup if warmup is None else warmup
        T, rows_all, _ = rows_for("c1" if small else "c2-real")
        T_job = sum(rows_all)
        if small:       # c1: the reference's 2-degree test grid, 100 block regions
            lat, lon, tas, df = synth.c1_workload(T=T)
            Gs, nlon = len(lat) * len(lon), len(lon)
            wname, lev = "areawt", "hierid"
            Xs = torch.from_numpy(np.ascontiguousarray(tas.reshape(T, Gs))).cuda()
        else:
            lat, lon, df = synth.realistic_segments(nlat=a.nlat, nlon=a.nlon, R=R, seed=2, land_frac=a.land_frac)
            Gs, nlon = G, a.nlon
            wname, lev = ("areawt" if dtype == "float32" else "popwt"), "hierid"
            Xs = engine.synth_field(T, Gs, seed=1000 + rank, base=280.0, amp=60.0, dtype=dtype)
        cell, codes, w_eff, uniq = synth.code_segments(df, lat, lon, wname, lev)
        t0 = time.perf_counter()
        plan = engine.SparsePlan(cell, codes, w_eff, Gs, len(uniq), row_len=nlon)
        plan_build_s = time.perf_counter() - t0
        Rr = len(uniq)
        st = stepper(lambda out: plan.apply(Xs, out=out), T, rows_all, Rr, Xs.dtype)
        prof = {"profile_reset": profile_reset, "profile_read": engine.profile_read} if a.full else {}
        dt, per_step, steps, warm_done = timed_steps(torch, dist, st.step, st.finish, steps, warmup, world, auto_steps=auto, **prof)
        if a.full:
            kst = kernel_stats(engine.profile_read(), steps, LAUNCHES_PER_APPLY)
            engine.profile_enable(False)
            kmed = kst["kernel_ms_median"] * 1e-3      # the roofline is priced on the MEDIAN launch
        if keep_out:
            keep_output(st)
        gok = gather_check(st, T)
        gt = gather_timing(st, T, per_step)
        plan.status()
        b = 4 if dtype == "float32" else 8
        nnz = plan.info["nnz"]
        wl = "c1" if small else ("c2-real" if dtype == "float32" else "c3-real")
        res = {
            "workload": wl, "dtype": "f32" if b == 4 else "f64", "T": T, "T_job": T_job, "G": Gs, "R": Rr, "nnz": int(nnz),
            "value": T_job * Gs * Rr * steps / dt, "unit": "gridcell-region-timesteps/s", "steps": steps, "warmup": warmup,
            "warmup_done": warm_done,
            "ms_per_step": dt / steps * 1e3, **step_stats(per_step), "nnz_timesteps_per_s": T_job * nnz * steps / dt,
            **({"gather_ok": gok} if gok is not None else {}), **gt,
            "plan_build_s": round(plan_build_s, 4),      # wagg_plan_create on the coded table (host-side chunking + upload), once per table
            "plan": {k: int(v) for k, v in plan.info.items()},
        }
        if a.full:
            abytes = sparse_algorithmic_bytes(T, Gs, Rr, nnz, b)
            traffic, tsrc = load_traffic(wl)
            kname = PLAN_KERNEL.get(int(plan.info.get("kernel_form", -1)),
                                    "sparse_lcv_kernel<float>" if b == 4 else "sparse_lcv_kernel<double>")
            res["roofline"] = net_of_events(on_traffic({"bound": "hbm", "achieved": abytes / kmed / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                        "frac": abytes / kmed / 1e9 / PEAK_HBM_GBS, "frac_basis": "median kernel time",
                                                        "traffic": traffic, "traffic_source": tsrc,
                                                        "kernel": kname, **kst, "algorithmic_bytes_per_launch": abytes},
                                                       kmed), abytes / 1e9, PEAK_HBM_GBS)
        if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
            Xh_cpu = Xs.cpu().numpy()
            res["cpu_baseline"] = cpu_baseline_sparse(Xh_cpu, cell, codes, w_eff, Rr, Gs,
                                                      "the FULL workload (all %d timesteps, full segment table)" % T)
            if not out_of_budget():
                res["cpu_baseline"]["reference_shaped"] = cpu_reference_shaped(Xh_cpu, lat, lon, df, wname, lev,
                                                                               budget_s=6.0 if small else a.ref_budget_s)
            del Xh_cpu
        if a.full and world == 1 and not small:
            # the same field in (gridcell, time) order -- the reference's (lat, lon, time) fixture layout
            XT = Xs.t().contiguous()
            gout = torch.empty((T, Rr), dtype=Xs.dtype, device="cuda")
            for _ in range(3):
                plan.apply(XT, layout="GT", out=gout)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                plan.apply(XT, layout="GT", out=gout)
            torch.cuda.synchronize()
            res["layout_gridcell_time"] = {"ms_per_step": (time.perf_counter() - t0) / steps * 1e3}
            del XT, gout
            # fused tas_poly: (tas - 273.15)^p, p = 1..4, one pass over the field
            pout = torch.empty((4, T, Rr), dtype=Xs.dtype, device="cuda")
            for _ in range(2):
                plan.apply_poly(Xs, -273.15, 4, out=pout)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                plan.apply_poly(Xs, -273.15, 4, out=pout)
            torch.cuda.synchronize()
            pdt = (time.perf_counter() - t0) / steps
            res["fused_tas_poly_1to4"] = {"ms_per_step": pdt * 1e3, "value": 4 * T * Gs * Rr / pdt,
                                          "unit": "gridcell-region-timesteps/s (4 powers)"}
            del pout
            # fused Snyder degree days: one pass over (tasmin, tasmax) for 1 and for 3 thresholds
            tmax = Xs + engine.synth_field(T, Gs, seed=2000 + rank, base=6.0, amp=10.0, dtype=dtype)
            edd = {}
            for K in (1, 3):
                thr = [10.0, 20.0, 30.0][:K]
                eout = torch.empty((K, T, Rr), dtype=Xs.dtype, device="cuda")
                for _ in range(2):
                    plan.apply_edd(Xs, tmax, thr, offset=-273.15, out=eout)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    plan.apply_edd(Xs, tmax, thr, offset=-273.15, out=eout)
                torch.cuda.synchronize()
                edd["K%d_ms" % K] = (time.perf_counter() - t0) / steps * 1e3
                del eout
            res["fused_snyder_edd"] = edd
            del tmax
        if a.full and world == 1 and not small and dtype == "float32":
            res.update(boundary_legs(Xs, lat, lon, df, plan, T, Gs, Rr))
            if "cpu_baseline" in res and "host_resident" in res:
                cb = res["cpu_baseline"]["cpu_best"]
                res["host_memory_comparison"] = {
                    "host_resident_gpu_ms": round(res["host_resident"]["ms_per_step"], 3),
                    "host_resident_gpu_lines_only_ms": round(res["host_resident"]["lines_only"]["ms_per_step"], 3),
                    "cpu_best_ms": round(cb["wall_s"] * 1e3, 3),
                    "cpu_best_min_ms": round(cb["wall_s_min"] * 1e3, 3), "cpu_threads": cb["cores"],
                    "device_resident_step_ms": round(res["median_ms"], 4),
                    "what": "for data that STARTS in host memory the GPU path is bound by PCIe (X crosses it once per call -- with "
                            "WAGG_HOST_LINES, the default of wagg_apply_host_* and the drop-in, only the 128-byte lines the table references, "
                            "packed by up to 12 host threads); "
                            "the all-cores CPU restatement reads X from DRAM.  The device-resident step beside them is what a "
                            "pipeline that keeps the field in HBM pays"}
        if a.full and world == 1 and not small and dtype == "float64":
            # the fp64 field (c3) in host memory: whole rows page-locked in place against lines only (47 % of a fp64 row)
            from climate_toolbox_amd import _lib as L_
            try:
                os.sched_setaffinity(0, AFFINITY_AT_START)           # (see boundary_legs: the OpenMP legs bound this thread)
            except (AttributeError, OSError, TypeError):
                pass
            Xh = Xs.cpu().numpy()
            hr = {}
            for name, flags in (("whole_rows_ms", L_.HOST_PIN), ("lines_only_ms", L_.HOST_PIN | L_.HOST_LINES)):
                ts = []
                for i in range(8):
                    t0 = time.perf_counter()
                    plan.apply_host(Xh, flags=flags)
                    ts.append((time.perf_counter() - t0) * 1e3)
                ts = sorted(ts[3:])
                hr[name] = ts[len(ts) // 2]
            hr["what"] = "wagg_apply_host_ex_f64 on the 3 GB field, result back in host memory (5 calls after 3 warm-up calls, medians)"
            res["host_resident"] = hr
            del Xh
        plan.close()
        return res

    cpu_dense_memo = {}
    c5_tables = {}                       # block-local? -> (rowptr, col, val) host CSR of the synthetic c5 table

    def run_dense_family(wl, plan=None, steps=None, warmup=None, keep_plan=False, share=False, auto=False, min_steps=10, keep_out=False):
        """c2-dense / c4 (full matrix), c5-uniform[-f64] (entry lists), c5-block[-f64] (tile-sparse)."""
        steps, warmup = steps or a.steps, a.warmup if warmup is None else warmup
        T, rows_all, scal = rows_for(wl, share)
        T_job = sum(rows_all)
        f64 = wl.endswith("-f64")
        dt_name = "float64" if f64 else "float32"
        X = engine.synth_field(T, G, seed=1000 + rank, base=280.0, amp=60.0, dtype=dt_name)
        build = None
        if wl.startswith("c5"):
            # configs[4] "sparse CSR weights": the table is HANDED IN as host CSR arrays (3 GB; here written by the
            # library's generator of the synthetic tables, outside the timed build) and the plan is what
            # wagg_dense_create_from_csr* makes of it -- bit-equal to the plan generated on the device from the same
            # hashes (tests/test_gpu_round4.py)
            bl = wl.startswith("c5-block")
            fill = 0.952 if bl else 0.01
            if plan is None:
                if bl not in c5_tables:
                    c5_tables.clear()                            # one table (3 GB of host memory) at a time
                    c5_tables[bl] = engine.synth_table_csr(G, R, 2, fill, blocklocal=bl)
                rowptr, col, val = c5_tables[bl]
                t0 = time.perf_counter()
                plan = engine.DensePlan.from_csr(rowptr, col, val, G, R, dtype=dt_name)
                build = {"plan_build_s": round(time.perf_counter() - t0, 4), "library_s": round(plan.info["build_s"], 4),
                         "upload_s": round(plan.info["build_upload_s"], 4), "table_entries": int(len(col)),
                         "table_bytes": int(rowptr.nbytes + col.nbytes + val.nbytes),
                         "one_pass_sort": int(plan.info["one_pass_sort"]),
                         "what": "wagg_dense_create_from_csr%s on host CSR arrays: upload, device sort (one stable pass per chunk of 128 "
                                 "cells for a table with ascending columns) + coalesce + denominators + form choice + packing" % ("_f64" if f64 else "")}
        else:
            fill, bl = 1.0, False
            plan = plan or engine.DensePlan.synth(G, R, seed=2)
        st = stepper(lambda out: plan.apply(X, out=out, ksplit=a.ksplit), T, rows_all, R, X.dtype)
        prof = {"profile_reset": profile_reset, "profile_read": engine.profile_read} if a.full else {}
        dt, per_step, steps, warm_done = timed_steps(torch, dist, st.step, st.finish, steps, warmup, world, auto_steps=auto,
                                                     min_steps=min_steps, **prof)
        if a.full:
            kst = kernel_stats(engine.profile_read(), steps, LAUNCHES_PER_APPLY)
            engine.profile_enable(False)
        if keep_out:
            keep_output(st)
        gok = gather_check(st, T)
        gt = gather_timing(st, T, per_step)
        form = int(plan.info["form"])
        if wl.startswith("c5-uniform"):
            nnz = int(plan.info["nnz"])
        elif wl.startswith("c5-block"):
            nnz = int(round(plan.info["n_tiles"] * (16 if f64 else 32) * 256 * fill))
        else:
            nnz = G * R
        res = {"workload": wl, "dtype": "f64" if f64 else "f32", "T": T, "T_job": T_job, "G": G, "R": R, "nnz": nnz,
               "value": T_job * G * R * steps / dt, "unit": "gridcell-region-timesteps/s", "steps": steps, "warmup": warmup,
               "warmup_done": warm_done,
               "ms_per_step": dt / steps * 1e3, **step_stats(per_step),
               "plan": {k: (int(v) if isinstance(v, int) else float("%.4g" % v)) for k, v in plan.info.items()}, "scaling": scal}
        if a.full:
            # one apply = one dominant-kernel launch (a full-form apply of several row blocks is one launch too); the roofline
            # is priced on the MEDIAN launch
            kmed = kst["kernel_ms_median"] * 1e-3
            flops = 2.0 * T * nnz                               # algorithmic: 2 T nnz (dense: nnz = G R)
            traffic, tsrc = load_traffic(wl)
            kname = {0: "dense_mfma_kernel", 1: "dense_pieces_kernel", 2: "spmm_kernel (vector ALU, entry lists)"}[form]
            if f64:
                kname = kname.replace("dense_mfma_kernel", "dense_mfma_kernel<double>").replace("dense_pieces_kernel", "dense_pieces_kernel<double>").replace("spmm_kernel", "spmm_kernel<double>")
            # entry lists run on the vector ALU: fp32 FMA peak = the fp32 MFMA peak (157.3), fp64 FMA = 78.6
            peak = PEAK_F64_MFMA_TFLOPS if f64 else PEAK_F32_MFMA_TFLOPS
            res["roofline"] = net_of_events({"bound": "mfma" if form != 2 else "valu", "achieved": flops / kmed / 1e12, "peak": peak,
                                             "unit": "TFLOP/s", "frac": flops / kmed / 1e12 / peak, "frac_basis": "median kernel time",
                                             "traffic": traffic, "traffic_source": tsrc, "kernel": kname,
                                             **kst, "algorithmic_flops_per_launch": flops}, flops / 1e12, peak)
        if gok is not None:
            res["gather_ok"] = gok
        res.update(gt)
        if build:
            res["plan_build"] = build
            res["plan_build_s"] = build["plan_build_s"]
        if wl != "c2-dense":
            res["rows"] = ("one rank's share: %d of the job's %d rows (shard 0 of %d)"
                           % (T, C4_TOTAL if wl == "c4" else C5_TOTAL, a.shards or 8)) if world == 1 else "rows %r" % (rows_all,)
        if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
            key = (fill, bl)                                    # c4 contracts the c2-dense operand: one CPU window serves both
            if key not in cpu_dense_memo:
                cpu_dense_memo[key] = cpu_baseline_dense(min(T, 365), G, R, 2, fill, bl)
            res["cpu_baseline"] = cpu_dense_memo[key]
        del X
        if not keep_plan:
            plan.close()
            plan = None
        return res, plan

    secondary = []

    def budgeted(wl, fn):
        """run a secondary unless the run's wall-clock budget is spent (the driver ends a run at 600 s; a line with a
        skipped entry beats no line)"""
        if out_of_budget():
            secondary.append({"workload": wl, "skipped": "budget", "elapsed_s": round(time.perf_counter() - t_start, 1),
                              "budget_s": a.budget_s})
            return None
        r = fn()
        secondary.append(r[0] if isinstance(r, tuple) else r)
        return r

    if a.workload in DENSE_FAMILY:
        want_secondary = a.full and a.workload == "c2-dense" and world == 1 and not a.no_secondary
        want_strong = a.full and a.workload == "c2-dense" and world > 1 and not a.no_secondary
        main_res, plan = run_dense_family(a.workload, keep_plan=want_secondary or want_strong, keep_out=bool(a.dump_outputs))
        scaling = main_res.get("scaling", "weak")
        if want_secondary:
            # every other BASELINE config on this GPU (N = 1): c4's rank share on the SAME 101 GB operand, then the rest.
            # SURVEY 8d's protocol for each: >= WARM_S of the same apply as warm-up, then max(10, what fills FILL_S) timed
            # steps (c4, 0.49 s per step: 5), median-based roofline, min / max / outlier flag in the entry.
            budgeted("c4", lambda: run_dense_family("c4", plan=plan, warmup=1, share=True, auto=True, min_steps=5))
            plan = None
            torch.cuda.empty_cache()
            budgeted("c2-real", lambda: run_sparse("float32", warmup=10, auto=True))     # segment-table form, fp32, area weights
            budgeted("c3-real", lambda: run_sparse("float64", warmup=10, auto=True))     # fp64 data, pop weights with backup fill
            budgeted("c1", lambda: run_sparse("float64", small=True, warmup=10, auto=True))
            for wl in ("c5-block", "c5-block-f64", "c5-uniform", "c5-uniform-f64"):
                torch.cuda.empty_cache()
                budgeted(wl, lambda wl=wl: run_dense_family(wl, warmup=2, share=True, auto=True))
        elif want_strong:
            # multi-GPU run: after the weak-scaled headline the STRONG splits of the two 8-GPU configs BASELINE names --
            # configs[3] (10,950 rows over the ranks, on the operand already resident) and configs[4] (18,250 rows,
            # entry lists) -- so that the scaling line speaks to them too.  Every rank takes part (the gather is inside).
            a_shards = a.shards
            a.shards = world
            budgeted("c4", lambda: run_dense_family("c4", plan=plan, steps=2, warmup=1))
            plan = None
            torch.cuda.empty_cache()
            budgeted("c5-uniform", lambda: run_dense_family("c5-uniform", steps=3, warmup=1))
            a.shards = a_shards
    elif a.workload == "c1":
        main_res = run_sparse("float64", small=True, keep_out=bool(a.dump_outputs))
    else:
        main_res = run_sparse("float32" if a.workload == "c2-real" else "float64", keep_out=bool(a.dump_outputs))
    T_job = main_res["T_job"]
    if a.dump_outputs and rank == 0:
        os.makedirs(a.dump_outputs, exist_ok=True)
        for name, arr in outputs.items():
            np.save(os.path.join(a.dump_outputs, name + ".npy"), arr)

    if rank == 0:
        wl = main_res["workload"]
        what = {"c1": "2-degree grid, 100 block regions, area-weighted, f64 (the reference's CPU-sized case)",
                "c2-dense": "area-weighted dense (gridcell x region) W, f32",
                "c4": "30-year daily series, dense W, f32", "c2-real": "area-weighted segment table, f32",
                "c3-real": "pop-weighted segment table with backup fill, f64",
                "c5-uniform": "ensemble x time rows, ~1 % of G x R non-zero at uniformly random positions, f32",
                "c5-block": "ensemble x time rows, ~1 % of G x R non-zero, block-local, f32",
                "c5-block-f64": "ensemble x time rows, ~1 % of G x R non-zero, block-local, f64",
                "c5-uniform-f64": "ensemble x time rows, ~1 % of G x R non-zero at uniformly random positions, f64"}[wl]
        line = {
            "metric": "gridcell-region-timesteps/sec", "value": main_res["value"],
            "unit": "gridcell-region-timesteps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": main_res["ms_per_step"], "median_ms": main_res.get("median_ms"), "min_ms": main_res.get("min_ms"),
            "higher_is_better": True, "scaling": scaling,
            **({"rehearsal": "WAGG_BENCH_REHEARSE=gloo: every rank on device 0, blocks gathered through host memory -- control flow "
                             "only, NOT a measurement"} if rehearse else {}),
            "scaling_measured": world > 1 and not rehearse,     # a one-GPU line says nothing about scaling; the driver computes efficiency from its N = 1, 2, 4, 8 runs
            "vs_baseline": None, "dtype": main_res["dtype"], "data": "synthetic",
            "config": {"workload": "%s: daily tas, T=%d rows on this GPU (%d in the job), grid G=%d, R=%d regions, %s; "
                                   "time axis sharded over %d GPU(s) + RCCL gather"
                                   % (wl, main_res["T"], T_job, main_res["G"], main_res["R"], what, world),
                       "T_per_gpu": main_res["T"], "T_job": T_job, "G": main_res["G"], "R": main_res["R"],
                       "parallelism": "time-shard x%d" % world},
            "roofline": main_res.get("roofline"),
            "cpu_baseline": main_res.get("cpu_baseline"),
        }
        for k in ("plan_build_s", "plan_build", "gather_ok", "host_resident", "dropin_ms", "agglev_ISO", "layout_gridcell_time",
                  "fused_tas_poly_1to4", "fused_snyder_edd", "host_memory_comparison"):
            if k in main_res:
                line[k] = main_res[k]
        if "nnz" in main_res:
            line["config"]["nnz"] = main_res["nnz"]
            line["config"]["plan"] = main_res["plan"]
        if rccl_ranks is not None:
            line["rccl_ranks"] = rccl_ranks
            for k in ("backend", "gather_ms", "gather_bytes", "per_rank_ms"):
                if k in main_res:
                    line[k] = main_res[k]
        line["warmup_done"] = main_res.get("warmup_done")
        line["max_ms"] = main_res.get("max_ms")
        line["step_outlier"] = main_res.get("step_outlier")
        line["elapsed_s"] = round(time.perf_counter() - t_start, 1)
        if secondary:
            line["secondary"] = secondary
        # the driver keeps the last 8 KB of stdout: one compact record per workload goes LAST, so every config's step,
        # kernel and roofline figures survive in that tail whatever the length of the entries above
        def brief(r):
            if "skipped" in r:
                return {"wl": r["workload"], "skipped": r["skipped"]}
            rf = r["roofline"]
            row = {"wl": r["workload"], "dtype": r["dtype"], "steps": r["steps"], "value": r["value"],
                   "step_ms": [round(r["median_ms"], 4), round(r["min_ms"], 4), round(r["max_ms"], 4)],
                   "kernel_ms": [round(rf["kernel_ms_median"], 4), round(rf["kernel_ms_min"], 4), round(rf["kernel_ms_max"], 4)],
                   "frac": round(rf["frac"], 4), "bound": rf["bound"]}
            if "frac_on_traffic" in rf:
                row["frac_on_traffic"] = round(rf["frac_on_traffic"], 4)
            if rf.get("kernel_ms_outlier") or r.get("step_outlier"):
                row["outlier"] = {"kernel": bool(rf.get("kernel_ms_outlier")), "step": bool(r.get("step_outlier"))}
            if "plan_build_s" in r:
                row["plan_build_s"] = r["plan_build_s"]
            cb = r.get("cpu_baseline")
            if cb:
                row["cpu_port_s"] = cb["wall_s"]
                rs = cb.get("reference_shaped")
                if rs:
                    row["cpu_reference_shaped_s"] = {"numpy": rs["numpy_scatter"]["wall_s"], "pandas": rs["pandas_groupby"]["wall_s"],
                                                     "rows_timed": [rs["numpy_scatter"]["rows_timed"], rs["pandas_groupby"]["rows_timed"]]}
            if "gather_ms" in r:
                row["gather_ms"] = round(r["gather_ms"], 3)
                row["gather_ok"] = r.get("gather_ok")
            return row
        rows = ([brief(main_res)] + [brief(r) for r in secondary]) if a.full else []
        if rows:
            line["summary"] = {"columns": "step_ms / kernel_ms = [median, min, max]; frac = roofline fraction on the median kernel time; "
                                          "cpu_port_s = oracle/wagg_oracle.c on its sample (1 thread for the segment-table rows); "
                                          "cpu_reference_shaped_s = the reference's NumPy / pandas shape, full workload (scaled from rows_timed)",
                               "rows": rows}
        # the reference-shaped CPU legs run on the segment-table workloads: the headline line names the c2-real pair at top level
        for r in rows:
            if r.get("wl") == "c2-real" and "cpu_reference_shaped_s" in r:
                line["cpu_reference_shaped_s"] = dict(r["cpu_reference_shaped_s"], workload="c2-real", c_port_s=r["cpu_port_s"],
                                                      gpu_step_s=round(r["step_ms"][0] * 1e-3, 7))
        emit(line, world, detail_files=a.full)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
