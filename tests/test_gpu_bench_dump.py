"""GPU tier: `bench.py --dump-outputs DIR` writes what the timed path computed in its last step.

The dump is the headline ensemble itself after the timed loop, so it is the same bits whatever --steps and --warmup are (every
step recomputes the whole axis from the same resident inputs), it is the oracle's bits for the sampled members (two-layer kind,
RSCM_MODE_EXACT: bit-exact, tests/test_gpu_parity.py), every value in it is finite (the sampled members that run away are in
status, not in the series), and it stays under 64 MB."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = 20_000    # more than bench.DUMP_MEMBERS: the seeded sample, not every member
NAMES = ("deep_ocean_temperature", "members", "status", "surface_temperature")


def _dump(out, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-extra",
           "--no-cpu-baseline", "--members", str(MEMBERS), "--details", str(out / "details.json"), "--dump-outputs", str(out / "dump")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(os.listdir(out / "dump")) == [n + ".npy" for n in NAMES]
    assert sum(os.path.getsize(out / "dump" / (n + ".npy")) for n in NAMES) <= 64 << 20
    return {n: np.load(out / "dump" / (n + ".npy")) for n in NAMES}


def test_bench_dump_is_the_last_timed_step(tmp_path):
    import bench
    from oracle import cbind
    from rscm_amd import _lib

    _lib.load()
    assert _lib.device_count() >= 1, "no HIP device visible"
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a = _dump(tmp_path / "a", 1, 0)
    b = _dump(tmp_path / "b", 3, 2)
    idx = bench.dump_sample(MEMBERS)
    assert len(idx) == bench.DUMP_MEMBERS and np.all(np.diff(idx) > 0) and idx[-1] < MEMBERS
    n_t = bench.T1 - bench.T0 + 1
    k = len(a["members"])
    for n in NAMES:
        assert a[n].dtype == np.float64 and np.isfinite(a[n]).all(), n
        assert a[n].shape == {"status": (len(idx),), "members": (k,)}.get(n, (n_t, k)), (n, a[n].shape)
        assert_bit_equal(a[n], b[n], f"{n}: --steps 1 --warmup 0 vs --steps 3 --warmup 2")

    # the same members through the oracle: bench.py's own ensemble gives their parameters
    ens = bench.make_ensemble(MEMBERS, 0, 0, 1, 0)
    P = ens.get_params()[:, idx]
    ens.close()
    t = np.arange(bench.T0, bench.T1 + 1, dtype=np.float64)
    want_ts, want_td = cbind.two_layer_run(np.append(t, t[-1] + 1.0), P, bench.f_syn(t), 0.0, 0.0, threads=8)
    failed = ~(np.isfinite(want_ts).all(axis=0) & np.isfinite(want_td).all(axis=0))
    assert np.array_equal(a["status"] != 0, failed) and 0 < failed.mean() < 0.1
    # the series are those of exactly the sampled members that stay finite, in sample order
    assert np.array_equal(a["members"], idx[~failed].astype(np.float64))
    assert_bit_equal(a["surface_temperature"], want_ts[:, ~failed], "Ts vs the oracle")
    assert_bit_equal(a["deep_ocean_temperature"], want_td[:, ~failed], "Td vs the oracle")
