"""CPU tier of the posterior resampling: the properties of the integer systematic draw on its numpy restatement
(tests/host_resample.py), the library's host-side offset against that restatement, and the product's 2-rank loop
(rscm_amd.distributed.resample_global / weights_stats_global) over a real gloo group with stand-in ensembles."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import host_resample as hr
from tests._dist_resample_worker import global_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    rng = np.random.default_rng(20261017)
    out = []
    for n, hi, M in [(1, 1 << 20, 7), (5, 4, 3), (40, 1 << 30, 40), (40, 1 << 30, 1), (300, 1 << 43, 1000), (300, 3, 50),
                     (1000, 1 << 20, 333), (64, 1 << 46, 4096)]:
        w = rng.integers(0, hi, size=n, dtype=np.int64)
        w[rng.random(n) < 0.3] = 0
        if not w.any():
            w[n // 2] = 1
        out.append((w, M))
    last = np.zeros(50, dtype=np.int64)
    last[-1] = 12345                      # all weight on the last member
    out.append((last, 17))
    big = np.zeros(8, dtype=np.int64)
    big[[1, 6]] = 1 << 52                 # W = 2^53, the bound of a handle's weights
    out.append((big, 1 << 20))
    return out


def _offsets(W, rng):
    return sorted({0, W - 1, W // 2, int(rng.integers(0, W))})


@pytest.mark.parametrize("case", range(len(_cases())))
def test_counts_points_and_zero_weights(case):
    w, M = _cases()[case]
    W = int(w.sum())
    rng = np.random.default_rng(case)
    for s in _offsets(W, rng):
        k_first, count, anc = hr.ancestors(w, M, s)
        assert (k_first, count) == (0, M)
        assert max(hr.points(M, s, W)) < W
        assert np.all(np.diff(anc) >= 0) and anc.min() >= 0 and anc.max() < len(w)
        assert np.all(w[anc] > 0)                                    # a zero-weight member is never drawn
        n = np.bincount(anc, minlength=len(w))
        for i, wi in enumerate(w):
            lo = (M * int(wi)) // W
            assert n[i] in (lo, lo + (1 if (M * int(wi)) % W else 0)), (i, n[i], lo)
        if M >= 1 << 12:
            assert np.array_equal(hr.ancestors_fast(w, M, s)[2], anc)


def test_one_draw_and_one_member():
    w = np.array([3, 0, 5, 2], dtype=np.int64)
    for s in range(10):
        assert hr.ancestors(w, 1, s)[2].tolist() == [0 if s < 3 else 2 if s < 8 else 3]
    k_first, count, anc = hr.ancestors(np.array([9], dtype=np.int64), 6, 4)
    assert (k_first, count) == (0, 6) and anc.tolist() == [0] * 6


@pytest.mark.parametrize("case", range(len(_cases())))
def test_shards_concatenate_to_the_whole(case):
    w, M = _cases()[case]
    W = int(w.sum())
    rng = np.random.default_rng(100 + case)
    for s in _offsets(W, rng):
        whole = hr.ancestors(w, M, s)[2]
        for _ in range(4):
            cuts = np.sort(rng.integers(0, len(w) + 1, size=int(rng.integers(1, 5))))
            edges = [0, *cuts.tolist(), len(w)]                      # repeated cuts: empty shards
            got, k_next, before = [], 0, 0
            for a, b in zip(edges[:-1], edges[1:]):
                k_first, count, anc = hr.ancestors(w[a:b], M, s, before, W)
                assert k_first == k_next or count == 0
                k_next = k_first + count if count else k_next
                got.append(anc + a)
                before += int(w[a:b].sum())
            assert k_next == M
            assert np.array_equal(np.concatenate(got), whole)


def test_offset_is_in_range_reproducible_and_the_library_agrees():
    from rscm_amd.ensemble import resample_offset
    seen = set()
    for seed in (0, 1, 2, 12345, (1 << 64) - 1, 0xDEADBEEFCAFEF00D):
        for W in (1, 2, 1000, (1 << 53), (1 << 53) - 111, (1 << 62) + 5):
            s = hr.offset(seed, W)
            assert 0 <= s < W and s == hr.offset(seed, W)
            assert resample_offset(seed, W) == s                     # rscm_gpu_resample_offset runs on the host
            seen.add((seed, s * (1 << 62) // W))
    assert len({v for _, v in seen}) > 6                             # different seeds land in different places
    from rscm_amd._lib import RscmGpuError
    with pytest.raises(RscmGpuError):
        resample_offset(1, 0)


def test_stats_are_exact():
    w = np.array([0, (1 << 52), 3, (1 << 52) - 1, 0, 7], dtype=np.int64)
    st = hr.stats(w)
    assert st["total"] == (1 << 53) + 9 and st["n_nonzero"] == 4 and st["w_max"] == 1 << 52
    assert st["sum_sq"] == (1 << 104) + 9 + ((1 << 52) - 1) ** 2 + 49
    assert st["ess"] == pytest.approx(2.0, rel=1e-12)
    assert hr.stats(np.zeros(3, dtype=np.int64))["ess"] == 0.0


@pytest.mark.parametrize("n_total,n_draws", [(9, 20), (1001, 400)])
def test_two_rank_gloo_resample(n_total, n_draws, tmp_path):
    seed = 777 + n_total
    port = str(29800 + n_total % 89)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_resample_worker.py"), str(n_total), str(n_draws), str(seed),
           str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = sorted((json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)), key=lambda x: x["rank"])
    w = global_weights(n_total)
    W = int(w.sum())
    k_first, count, whole = hr.ancestors(w, n_draws, hr.offset(seed, W))
    assert (k_first, count) == (0, n_draws)
    assert res[0]["k_first"] == 0 and res[1]["k_first"] == res[0]["count"] and res[0]["count"] + res[1]["count"] == n_draws
    got = np.concatenate([np.array(x["ancestors"], dtype=np.int64) + x["offset"] for x in res])
    assert np.array_equal(got, whole)
    want = hr.stats(w)
    for x in res:
        assert x["world"] == 2
        assert {k: (v if k == "ess" else int(v)) for k, v in x["stats"].items()} == want
