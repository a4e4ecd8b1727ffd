"""bench.py without --full (run with -m gpu on an MI355X): a plain run times exactly --steps steps of the headline workload
and nothing else, and --dump-outputs writes what its last timed step computed -- the oracle's numbers for the same seeded
inputs, the same from run to run, and a seeded row sample when the output is larger than bench.DUMP_LIMIT."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, _rel_ok

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--workload", "c2-real", "--nlat", "180", "--nlon", "360", "--R", "600", "--warmup", "1"]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    from tests.bench_io import split_bench_output
    return split_bench_output(p)


def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    line, rec = _bench(*SMALL, "--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    assert line["steps"] == rec["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None and "summary" not in line
    assert not any(k in rec for k in ("secondary", "host_resident", "dropin_ms", "layout_gridcell_time", "fused_tas_poly_1to4"))
    got = np.load(tmp_path / "a" / "out.npy")
    assert got.dtype == np.float32 and got.shape == (365, rec["config"]["R"])
    # the seeded inputs of the run, rebuilt here: the dump is the oracle's aggregation of them
    import torch
    from climate_toolbox_amd import engine, synth
    from oracle import ref_numpy as O
    lat, lon, df = synth.realistic_segments(nlat=180, nlon=360, R=600, seed=2, land_frac=0.30)
    cell, codes, w_eff, uniq = synth.code_segments(df, lat, lon, "areawt", "hierid")
    X = engine.synth_field(365, 180 * 360, seed=1000, base=280.0, amp=60.0, dtype="float32").cpu().numpy()
    torch.cuda.synchronize()
    _rel_ok(got, O.agg_coded(X, cell, codes, w_eff, len(uniq)), RTOL32)
    # the same arguments give the same inputs: another build (here the same one) can be compared output for output
    line2, _ = _bench(*SMALL, "--steps", "5", "--dump-outputs", str(tmp_path / "b"))
    assert line2["steps"] == 5
    _rel_ok(np.load(tmp_path / "b" / "out.npy"), got, 1e-6)


def test_dump_of_a_large_output_is_a_seeded_row_sample(tmp_path):
    import bench
    T = 30000                                           # 30,000 x 600 fp32 = 72 MB > DUMP_LIMIT
    _bench(*SMALL, "--T", str(T), "--steps", "1", "--dump-outputs", str(tmp_path))
    got = np.load(tmp_path / "out.npy")
    assert got.nbytes <= bench.DUMP_LIMIT and got.shape[0] == bench.DUMP_LIMIT // (got.shape[1] * 4) < T
    assert np.isfinite(got).any()
