"""Member sharding across the GPUs of one node.

Members are independent (each ``run`` builds its own model,
crates/rscm-calibrate/src/model_runner.rs:257-266), so the ensemble shards embarrassingly:
rank ``g`` of ``G`` owns the contiguous global members ``[offset, offset+count)``, keeps its SoA
buffers in its own HBM and runs the same kernels.  There is NO data-path collective.  The only
exchanges, over ``torch.distributed`` (backend ``nccl`` = RCCL over xGMI on the GPU box, ``gloo``
in the CPU tests), are:

* ``gather_members``: all-gather of one small per-member vector (log-likelihood, status) --
  8 B per member, e.g. 8 MB for 1e6 members;
* ``reduce_summary``: all-reduce of count/sum/min/max;
* ``quantile_rows_global``: eight all-reduces (int64 SUM) of radix-select histograms -- a few
  hundred counts per row and quantile, however many members there are (weight sums instead of
  counts for the likelihood-weighted quantiles);
* ``ShardedEnsemble.constrain``: one all-reduce (MAX) of the local log-likelihood maxima;
* ``quantile_vectors_global``: the same histogram all-reduces over per-member vectors (indicators, parameter rows);
* ``exceedance_global``: one all-reduce (int64 SUM) of the exceedance counts or weight sums;
* ``moments_global``: two all-reduces (int64 SUM) of the fixed-point moment sums, 69 int64 per mean and covariance entry;
* ``moment_rows_global``: the same two all-reduces for the mean and spread of a stored variable at every row;
* ``histogram_rows_global``, ``histogram_vectors_global``, ``histogram2d_global``: one all-reduce (int64 SUM) of the bin sums;
* ``exceedance_rows_global``, ``rank_rows_global``: one all-reduce (int64 SUM) of the per-row hits, equals and totals;
* ``weights_stats_global``: one all-reduce (int64 SUM) of the exact weight sums and one (MAX) of the largest weight;
* ``resample_global``: one all-gather of each rank's exact summed weight (8 B per rank); no member crosses a rank.

Baselines and per-member indicators (``Ensemble.set_baseline``, ``Ensemble.indicators``) are per member and need none.

Full time series are never gathered: 12 GB into one GPU's seven xGMI links would serialise on
rank 0 for no benefit; each rank copies its own shard to the host if asked.
Parameters need no scatter either: ``Ensemble.sample_lhs`` is counter-based on the global
member id, so every rank generates its own rows of one global Latin hypercube.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np


def shard_bounds(n_total: int, rank: int, world: int) -> Tuple[int, int]:
    """(offset, count) of rank's contiguous member block; blocks differ by at most one member."""
    if not (0 <= rank < world) or n_total < 0:
        raise ValueError("bad rank/world/n_total")
    base, rem = divmod(n_total, world)
    count = base + (1 if rank < rem else 0)
    offset = rank * base + min(rank, rem)
    return offset, count


def env_rank_world() -> Tuple[int, int, int]:
    """(rank, local_rank, world) from the torchrun environment (defaults: single process)."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def _dist():
    import torch.distributed as dist
    return dist


def is_distributed() -> bool:
    """An initialised process group of more than one rank -- or of one rank when
    ``RSCM_FORCE_DISTRIBUTED=1`` (rehearsal of the collective paths, e.g. RCCL on a one-GPU box)."""
    try:
        d = _dist()
        if not (d.is_available() and d.is_initialized()):
            return False
        return d.get_world_size() > 1 or os.environ.get("RSCM_FORCE_DISTRIBUTED") == "1"
    except Exception:
        return False


def _device_for_backend():
    import torch
    d = _dist()
    if d.get_backend() == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def gather_members(local, n_total: int, group=None) -> np.ndarray:
    """All-gather a per-member vector sharded by ``shard_bounds`` into the global order.
    Every rank returns the full ``[n_total]`` array on the host.

    ``local`` is a numpy array or a ``DeviceVector`` (``Ensemble.loglik(..., on_device=True)``,
    ``status_device()``).  With the ``nccl`` backend a device vector is gathered where it lies: one
    device-to-device copy into the padded send buffer, the RCCL all-gather, one copy of the gathered
    vector to the host -- no host round trip of the shard.  With ``gloo`` (CPU rehearsals) the shard
    comes to the host first."""
    from .ensemble import DeviceVector
    on_device = isinstance(local, DeviceVector)
    if not is_distributed():
        host = local.to_host() if on_device else np.ascontiguousarray(local).copy()
        if len(host) != n_total:
            raise ValueError("single process: local shard must be the whole ensemble")
        return host
    import torch
    d = _dist()
    world, rank = d.get_world_size(group), d.get_rank(group)
    off, cnt = shard_bounds(n_total, rank, world)
    if len(local) != cnt:
        raise ValueError(f"rank {rank}: shard has {len(local)} members, expected {cnt}")
    dev = _device_for_backend()
    max_cnt = shard_bounds(n_total, 0, world)[1]
    if on_device and dev.type == "cuda":
        src = torch.as_tensor(local, device=dev)            # zero-copy view of the library's buffer
        mine = torch.zeros(max_cnt, dtype=src.dtype, device=dev)
        mine[:cnt].copy_(src)
    else:
        host = local.to_host() if on_device else np.ascontiguousarray(local)
        pad = np.zeros(max_cnt, dtype=host.dtype)
        pad[:cnt] = host
        mine = torch.from_numpy(pad).to(dev)
    gathered = torch.empty(world * max_cnt, dtype=mine.dtype, device=dev)
    d.all_gather_into_tensor(gathered, mine, group=group)
    parts = gathered.cpu().numpy().reshape(world, max_cnt)
    out = np.empty(n_total, dtype=parts.dtype)
    for r in range(world):
        o, c = shard_bounds(n_total, r, world)
        out[o:o + c] = parts[r, :c]
    return out


def reduce_summary(local: Dict[str, float], group=None) -> Dict[str, float]:
    """Combine ``Ensemble.summary`` dicts (count, mean, min, max) over ranks."""
    cnt = float(local["count"])
    s = local["mean"] * cnt if cnt else 0.0
    if not is_distributed():
        return dict(local)
    import torch
    d = _dist()
    dev = _device_for_backend()
    acc = torch.tensor([cnt, s], dtype=torch.float64, device=dev)
    mn = torch.tensor([local["min"]], dtype=torch.float64, device=dev)
    mx = torch.tensor([local["max"]], dtype=torch.float64, device=dev)
    d.all_reduce(acc, op=d.ReduceOp.SUM, group=group)
    d.all_reduce(mn, op=d.ReduceOp.MIN, group=group)
    d.all_reduce(mx, op=d.ReduceOp.MAX, group=group)
    total = float(acc[0].item())
    return {"count": int(total), "mean": float(acc[1].item()) / total if total else float("nan"),
            "min": float(mn.item()), "max": float(mx.item())}


def _reduce_select(sel, group=None) -> Dict[str, np.ndarray]:
    """Runs a staged select (``QuantileSelect`` or a stand-in) to its result, SUM-all-reducing each pass's int64 buffer."""
    import torch
    from .ensemble import DeviceVector
    d = _dist()
    dev = _device_for_backend()
    with sel as s:
        while True:
            buf = s.next_pass()
            if buf is None:
                break
            if isinstance(buf, DeviceVector) and dev.type == "cuda":
                t = torch.as_tensor(buf, device=dev)            # zero-copy view of the library's buffer
                d.all_reduce(t, op=d.ReduceOp.SUM, group=group)
                torch.cuda.current_stream(dev).synchronize()    # the commit runs on the ensemble's stream
                s.commit()
            else:
                host = buf.to_host() if isinstance(buf, DeviceVector) else np.ascontiguousarray(buf, dtype=np.int64)
                t = torch.from_numpy(host.copy()).to(dev)
                d.all_reduce(t, op=d.ReduceOp.SUM, group=group)
                s.commit(t.cpu().numpy())
        return s.result()


def quantile_rows_global(ensemble, var, q, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                         group=None, weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """Quantiles of the WHOLE sharded ensemble (``Ensemble.quantile_rows`` of all ranks' members together), on every rank.

    Each rank runs the staged radix select on its own shard (``Ensemble.select``); between the passes the ranks sum their
    int64 histograms -- the only collective, exact and independent of order, so the result has the same bits at any number
    of ranks and equals the single-process ``quantile_rows`` of the gathered ensemble.  With ``nccl`` the library's buffer is
    reduced in place through ``__cuda_array_interface__``; with ``gloo`` it goes through the host.  Every rank must pass the
    same ``q`` and rows and stand at the same time index.  Single process: ``ensemble.quantile_rows``.

    ``weighted``: the likelihood-weighted quantiles (``Ensemble.quantile_rows(..., weighted=True)``) of the whole ensemble,
    the ranks' member weights on one scale (``ShardedEnsemble.constrain``); the histograms then hold int64 weight sums and
    the result has ``"weight"`` in place of ``"count"``.

    ``anomaly``: of each member's anomaly against its baseline (every rank's ``Ensemble.set_baseline`` over the same rows).

    ``grouped``: per member group (every rank's ``Ensemble.set_member_groups`` for its own members, with the same ``n_groups``
    on every rank; a rank may hold no member of a group): the buffers carry one histogram per group, the result is group-major."""
    # a keyword goes to the ensemble only when set: an ensemble-like object that has no weighted, anomaly or grouped form need not take it
    kw = {}
    if weighted:
        kw["weighted"] = True
    if anomaly:
        kw["anomaly"] = True
    if grouped:
        kw["grouped"] = True
    if not is_distributed():
        return ensemble.quantile_rows(var, q, t_begin, t_end, t_stride, **kw)
    return _reduce_select(ensemble.select(var, q, t_begin, t_end, t_stride, **kw), group)


def quantile_vectors_global(ensemble, vectors, q, group=None, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.quantile_vectors`` of the WHOLE sharded ensemble on every rank: each rank passes its shard of each vector
    (its members' indicators, parameter rows ...) in the same order; the histograms are summed as in ``quantile_rows_global``."""
    kw = {"grouped": True} if grouped else {}
    if not is_distributed():
        return ensemble.quantile_vectors(vectors, q, weighted=weighted, **kw)
    return _reduce_select(ensemble.select_vectors(vectors, q, weighted=weighted, **kw), group)


def _all_reduce_sum(a, group=None) -> np.ndarray:
    """The int64 array ``a`` summed element by element over the ranks (exact and independent of order); single process: ``a``.
    With ``gloo`` the array passes through the host."""
    a = np.ascontiguousarray(a, dtype=np.int64)
    if not is_distributed():
        return a
    import torch
    d = _dist()
    t = torch.from_numpy(a.copy()).to(_device_for_backend())
    d.all_reduce(t, op=d.ReduceOp.SUM, group=group)
    return t.cpu().numpy()


def exceedance_global(ensemble, vector, thresholds, group=None, weighted: bool = False, grouped: bool = False) -> Dict[str, object]:
    """``Ensemble.exceedance`` of the WHOLE sharded ensemble on every rank: the ranks' int64 hits and totals are SUM-reduced
    (exact and independent of order), then ``probability = hits / total``.  ``grouped``: per member group, ``[G][k] + [G]`` int64
    in one reduction (the same ``n_groups`` on every rank)."""
    from .ensemble import exceedance_grouped_result, exceedance_result
    local = ensemble.exceedance(vector, thresholds, weighted=weighted, **({"grouped": True} if grouped else {}))
    if not is_distributed():
        return local
    hits = np.asarray(local["hits"], dtype=np.int64)
    acc = _all_reduce_sum(np.append(hits.ravel(), np.asarray(local["total"], dtype=np.int64)), group)   # [G][k] + [G], or [k] + 1
    if grouped:
        return exceedance_grouped_result(acc[:hits.size].reshape(hits.shape), acc[hits.size:])
    return exceedance_result(acc[:-1], int(acc[-1]))


def _moments_reduced(sums, means, result, K: int, group, grouped: bool):
    """The two collectives of the global moments: ``sums(order, center)`` of order 1 are reduced and finished into the means, the
    sums of order 2 about them are reduced, and ``result`` finishes both.  G is the axis before the last of the sums."""
    sums1 = _all_reduce_sum(sums(1, None), group)
    G = sums1.shape[-2]
    sums2 = _all_reduce_sum(sums(2, means(sums1, K, G)), group)
    return result(sums1, sums2, K, G, grouped=grouped)


def moments_global(ensemble, vectors, group=None, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.moments`` of the WHOLE sharded ensemble on every rank: each rank forms the order-1 sums of its shard of each
    vector (``Ensemble.moment_sums``), the int64 arrays are SUM-reduced and every rank finishes the same means; then the order-2
    sums about those means, reduced and finished the same way.  The sums are integers with deferred carries, exact and
    independent of order, so the result has the same bits at any number of ranks and equals ``Ensemble.moments`` of the gathered
    ensemble.  Two collectives and no data-path copy (with ``gloo`` the two small arrays pass through the host).  ``grouped``:
    the same ``n_groups`` on every rank.  Fewer than 2^31 members may count over all ranks."""
    from .ensemble import moment_means, moments_result
    vs = list(vectors)
    kw = {"grouped": True} if grouped else {}
    return _moments_reduced(lambda order, center: ensemble.moment_sums(vs, order, center=center, weighted=weighted, **kw),
                            moment_means, moments_result, len(vs), group, grouped)


def moment_rows_global(ensemble, var, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, vectors=(), group=None,
                       weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.moment_rows`` of the WHOLE sharded ensemble on every rank, exactly as ``moments_global`` proceeds: each rank forms
    the order-1 sums of its shard (``Ensemble.moment_rows_sums``), the int64 arrays are SUM-reduced and every rank finishes the same
    means; then the order-2 sums about those means, reduced and finished the same way.  Two collectives; the result has the same bits
    at any number of ranks and equals ``Ensemble.moment_rows`` of the gathered ensemble.  Every rank passes the same rows and its
    shard of each vector in the same order and stands at the same time index; ``grouped``: the same ``n_groups`` on every rank.
    Fewer than 2^31 members may count in a row over all ranks."""
    from .ensemble import moment_rows_means, moment_rows_result
    vs = list(vectors)
    kw = {}
    if weighted:
        kw["weighted"] = True
    if anomaly:
        kw["anomaly"] = True
    if grouped:
        kw["grouped"] = True
    return _moments_reduced(lambda order, center: ensemble.moment_rows_sums(var, order, t_begin, t_end, t_stride, vectors=vs, center=center, **kw),
                            moment_rows_means, moment_rows_result, len(vs), group, grouped)


def _row_flags(weighted: bool, anomaly: bool, grouped: bool) -> Dict[str, bool]:
    """A keyword goes to the ensemble only when set, as in ``quantile_rows_global``."""
    return {k: True for k, v in (("weighted", weighted), ("anomaly", anomaly), ("grouped", grouped)) if v}


def _reduce_together(arrays, group=None):
    """The int64 arrays SUM-reduced in ONE collective (concatenated, then cut back to their shapes)."""
    arrays = [np.asarray(a, dtype=np.int64) for a in arrays]
    acc = _all_reduce_sum(np.concatenate([a.ravel() for a in arrays]), group)
    cuts = np.cumsum([a.size for a in arrays])[:-1]
    return [part.reshape(a.shape) for part, a in zip(np.split(acc, cuts), arrays)]


def exceedance_rows_global(ensemble, var, thresholds, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, group=None,
                           weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.exceedance_rows`` of the WHOLE sharded ensemble on every rank: the ranks' int64 hits and totals of every row are
    SUM-reduced in one collective (exact and independent of order), then ``ensemble.exceedance_rows_result`` forms the
    probabilities.  Every rank passes the same rows and thresholds and stands at the same time index; ``grouped``: the same
    ``n_groups`` on every rank."""
    from .ensemble import exceedance_rows_result
    local = ensemble.exceedance_rows(var, thresholds, t_begin, t_end, t_stride, **_row_flags(weighted, anomaly, grouped))
    hits, total = _reduce_together([local["hits"], local["total"]], group)
    return exceedance_rows_result(hits, total, grouped)


def rank_rows_global(ensemble, var, record, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, group=None,
                     weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.rank_rows`` of the WHOLE sharded ensemble on every rank: the ranks' int64 sums below, equal to and around the
    record at every row are SUM-reduced in one collective, then ``ensemble.rank_rows_result`` forms the mid-rank.  Every rank
    passes the same rows and record."""
    from .ensemble import rank_rows_result
    local = ensemble.rank_rows(var, record, t_begin, t_end, t_stride, **_row_flags(weighted, anomaly, grouped))
    below, equal, total = _reduce_together([local["below"], local["equal"], local["total"]], group)
    return rank_rows_result(total - below, equal, total, record, grouped)


def histogram_rows_global(ensemble, var, edges, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, group=None,
                          weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.histogram_rows`` of the WHOLE sharded ensemble on every rank: the ranks' int64 counts, below, above and totals of
    every row are SUM-reduced in one collective (exact and independent of order), then ``ensemble.histogram_result`` forms the
    probabilities.  Every rank passes the same rows and edges and stands at the same time index; ``grouped``: the same ``n_groups``
    on every rank."""
    from .ensemble import histogram_result
    local = ensemble.histogram_rows(var, edges, t_begin, t_end, t_stride, **_row_flags(weighted, anomaly, grouped))
    return histogram_result(*_reduce_together([local[k] for k in ("counts", "below", "above", "total")], group), grouped)


def histogram_vectors_global(ensemble, vectors, edges, group=None, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.histogram_vectors`` of the WHOLE sharded ensemble on every rank: one SUM-reduction of the int64 sums, then
    ``ensemble.histogram_result``.  Every rank passes its shard of each vector in the same order, and the same edges."""
    from .ensemble import histogram_result
    local = ensemble.histogram_vectors(list(vectors), edges, **_row_flags(weighted, False, grouped))
    return histogram_result(*_reduce_together([local[k] for k in ("counts", "below", "above", "total")], group), grouped)


def histogram2d_global(ensemble, x, y, edges_x, edges_y, group=None, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
    """``Ensemble.histogram2d`` of the WHOLE sharded ensemble on every rank: one SUM-reduction of the int64 counts, outside and
    totals, then ``ensemble.histogram2d_result``.  Every rank passes its shard of the two vectors and the same edges."""
    from .ensemble import histogram2d_result
    local = ensemble.histogram2d(x, y, edges_x, edges_y, **_row_flags(weighted, False, grouped))
    return histogram2d_result(*_reduce_together([local[k] for k in ("counts", "outside", "total")], group), grouped)


def weights_stats_global(ensemble, group=None) -> Dict[str, object]:
    """``Ensemble.weights_stats`` of the WHOLE sharded ensemble on every rank: the ranks' exact integers are SUM-reduced (``w_max``:
    MAX) -- sum w^2 as four 32-bit limbs, each of which sums without wrapping over any number of ranks an int64 can count -- and
    the effective sample size is formed once from the reduced integers."""
    from .ensemble import weights_stats_result
    local = ensemble.weights_stats()
    if not is_distributed():
        return local
    import torch
    d = _dist()
    dev = _device_for_backend()
    sq = int(local["sum_sq"])
    limbs = [(sq >> (32 * k)) & 0xFFFFFFFF for k in range(4)]
    t = torch.tensor([int(local["total"]), int(local["n_nonzero"])] + limbs, dtype=torch.int64, device=dev)
    m = torch.tensor([int(local["w_max"])], dtype=torch.int64, device=dev)
    d.all_reduce(t, op=d.ReduceOp.SUM, group=group)
    d.all_reduce(m, op=d.ReduceOp.MAX, group=group)
    acc = [int(x) for x in t.cpu().numpy()]
    return weights_stats_result(acc[0], acc[1], int(m.item()), sum(acc[2 + k] << (32 * k) for k in range(4)))


def resample_global(ensemble, n_draws: int, seed: int = 0, group=None, offset: Optional[int] = None):
    """This rank's share of ONE systematic draw of ``n_draws`` members from the whole sharded ensemble's weights:
    ``(k_first, count, ancestors)`` -- the contiguous run of draws whose ancestors this rank owns and their LOCAL member
    indices (``Ensemble.resample``: an int64 device vector).  The ranks all-gather their exact summed weights (rank order is
    member order), every rank derives the same offset from ``seed``, and the rest is integer arithmetic per rank: the runs of
    all ranks concatenate to the draw a single process makes from the gathered weights, bit for bit, at any number of ranks.
    A rank's posterior shard is the draws it owns; shards are of unequal size and no member crosses a rank."""
    from .ensemble import resample_offset
    w_local = int(ensemble.weights_stats()["total"])
    if not is_distributed():
        w_before, w_total = 0, w_local
    else:
        import torch
        d = _dist()
        world, rank = d.get_world_size(group), d.get_rank(group)
        dev = _device_for_backend()
        mine = torch.tensor([w_local], dtype=torch.int64, device=dev)
        gathered = torch.empty(world, dtype=torch.int64, device=dev)
        d.all_gather_into_tensor(gathered, mine, group=group)
        totals = [int(x) for x in gathered.cpu().numpy()]
        w_before, w_total = sum(totals[:rank]), sum(totals)
    if w_total <= 0:
        raise ValueError("the member weights of the whole ensemble sum to zero: nothing to draw from")
    if offset is None:
        offset = resample_offset(seed, w_total)
    anc = ensemble.resample(n_draws, offset=offset, w_before=w_before, w_total=w_total)
    return anc.k_first, len(anc), anc


class ShardedEnsemble:
    """One global ensemble of ``n_total`` members, this rank holding its block on its GPU.

    ``factory(count, device)`` must return a configured ``rscm_amd.Ensemble`` of ``count`` members
    (forcing and initial values set); parameters are then drawn on the device from one global
    Latin hypercube, or set from the rank's slice of a global matrix.
    """

    def __init__(self, n_total: int, factory, rank: Optional[int] = None,
                 world: Optional[int] = None, device: Optional[int] = None):
        r, lr, w = env_rank_world()
        self.rank = r if rank is None else rank
        self.world = w if world is None else world
        self.n_total = int(n_total)
        self.offset, self.count = shard_bounds(self.n_total, self.rank, self.world)
        self.ensemble = factory(self.count, lr if device is None else device)

    def sample_lhs(self, seed: int, low, high) -> None:
        self.ensemble.sample_lhs(seed, low, high, self.offset, self.n_total)

    def sample_lhs_priors(self, seed: int, priors, base=None) -> None:
        """This shard's block of the global hypercube through the rows' priors (``Ensemble.sample_lhs_priors``)."""
        self.ensemble.sample_lhs_priors(seed, priors, base, self.offset, self.n_total)

    def set_forcing_noise(self, sigma: float, seed: int, phi: float = 0.0) -> None:
        """Forcing noise of the global ensemble (``Ensemble.set_forcing_noise``, red with ``phi != 0``): the shard's first member
        is the offset, so a member draws the same variability whichever rank holds it."""
        self.ensemble.set_forcing_noise(sigma, seed, self.offset, phi)

    def set_forcing_noise_members(self, seed: int) -> None:
        """Per-member forcing noise of the global ensemble (``Ensemble.set_forcing_noise_members``): the shard's first member is
        the offset; the amplitude and persistence rows are the shard's slice of the global parameter block."""
        self.ensemble.set_forcing_noise_members(seed, self.offset)

    def set_params_global(self, soa: np.ndarray) -> None:
        self.ensemble.set_params(np.ascontiguousarray(soa[:, self.offset:self.offset + self.count]))

    def run(self) -> None:
        self.ensemble.rewind()
        self.ensemble.run()

    def loglik_global(self, obs_var, obs_tidx, obs_value, obs_sigma, normalize=False, reference=None) -> np.ndarray:
        local = self.ensemble.loglik(obs_var, obs_tidx, obs_value, obs_sigma, normalize, on_device=True, reference=reference)
        return gather_members(local, self.n_total)

    def status_global(self) -> np.ndarray:
        return gather_members(self.ensemble.status_device(), self.n_total)

    def params_global(self) -> np.ndarray:
        """The global ``[P][n_total]`` parameter matrix (one gather per row)."""
        P = self.ensemble.get_params()
        return np.stack([gather_members(np.ascontiguousarray(row), self.n_total) for row in P])

    def summary_global(self, var, tidx: int) -> Dict[str, float]:
        return reduce_summary(self.ensemble.summary(var, tidx))

    def define_diagnostic(self, name: str, terms) -> int:
        """``Ensemble.define_diagnostic`` on this rank's block.  The combination is per member, so the shards' rows are the
        whole ensemble's and no collective is needed; ``quantile_rows_global`` and ``constrain`` then take the name."""
        return self.ensemble.define_diagnostic(name, terms)

    def define_energy_budget(self, quantity: str, name: Optional[str] = None, scale: float = 1.0) -> int:
        """``Ensemble.define_energy_budget`` on this rank's block.  The quantities are per member; a shard's forcing noise is drawn
        for its members' ids in the whole ensemble (the block's member offset, as in its run), so the shards' rows are the whole
        ensemble's."""
        return self.ensemble.define_energy_budget(quantity, name, scale)

    def define_running_mean(self, name: str, source, window: int = 20, align: str = "centre", step: int = 1) -> int:
        """``Ensemble.define_running_mean`` on this rank's block.  The mean is per member, so the shards' rows are the blocks of
        the whole ensemble's."""
        return self.ensemble.define_running_mean(name, source, window, align, step)

    def compute_diagnostic(self, var, t_begin: Optional[int] = None, t_end: Optional[int] = None, t_stride: int = 1) -> None:
        """``Ensemble.compute_diagnostic`` on this rank's block; every rank calls it with the same range."""
        self.ensemble.compute_diagnostic(var, t_begin, t_end, t_stride)

    def quantile_rows_global(self, var, q, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                             weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Quantiles of the global ensemble at the rows ``t_begin, t_begin + t_stride, ... < t_end`` (``quantile_rows_global``);
        ``weighted``: with the member weights ``constrain`` set; ``anomaly``: of the anomalies against the members' baselines;
        ``grouped``: per member group."""
        return quantile_rows_global(self.ensemble, var, q, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, grouped=grouped)

    def quantile_vectors_global(self, vectors, q, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Quantiles of per-member vectors of the global ensemble (``quantile_vectors_global``)."""
        return quantile_vectors_global(self.ensemble, vectors, q, weighted=weighted, grouped=grouped)

    def moments_global(self, vectors, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Exact means, covariances and correlations of per-member vectors over the global ensemble (``moments_global``)."""
        return moments_global(self.ensemble, vectors, weighted=weighted, grouped=grouped)

    def moment_rows_global(self, var, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, vectors=(), weighted: bool = False,
                           anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Exact mean and spread of a stored variable at every row over the global ensemble, with its covariance with per-member
        vectors (``moment_rows_global``)."""
        return moment_rows_global(self.ensemble, var, t_begin, t_end, t_stride, vectors, weighted=weighted, anomaly=anomaly, grouped=grouped)

    def exceedance_rows_global(self, var, thresholds, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                               weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Exceedance probabilities of a stored variable at every row over the global ensemble (``exceedance_rows_global``)."""
        return exceedance_rows_global(self.ensemble, var, thresholds, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly,
                                      grouped=grouped)

    def rank_rows_global(self, var, record, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                         anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Where a record lies inside the global ensemble's plume at every row (``rank_rows_global``)."""
        return rank_rows_global(self.ensemble, var, record, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, grouped=grouped)

    def histogram_rows_global(self, var, edges, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                              anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """The histogram of a stored variable at every row over the global ensemble (``histogram_rows_global``)."""
        return histogram_rows_global(self.ensemble, var, edges, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, grouped=grouped)

    def histogram_vectors_global(self, vectors, edges, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Histograms of per-member vectors over the global ensemble (``histogram_vectors_global``)."""
        return histogram_vectors_global(self.ensemble, vectors, edges, weighted=weighted, grouped=grouped)

    def histogram2d_global(self, x, y, edges_x, edges_y, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """The joint histogram of two per-member vectors over the global ensemble (``histogram2d_global``)."""
        return histogram2d_global(self.ensemble, x, y, edges_x, edges_y, weighted=weighted, grouped=grouped)

    def exceedance_global(self, vector, thresholds, weighted: bool = False, grouped: bool = False) -> Dict[str, object]:
        """Exceedance probabilities of a per-member vector over the global ensemble (``exceedance_global``)."""
        return exceedance_global(self.ensemble, vector, thresholds, weighted=weighted, grouped=grouped)

    def constrain(self, obs_var, obs_tidx, obs_value, obs_sigma, normalize: bool = False, bits: Optional[int] = None, reference=None):
        """Weight this rank's members by their fit to observations, on one scale across all ranks: the Gaussian
        log-likelihood on the device, a MAX all-reduce of the local maxima, then ``set_weights_from_loglik`` with the global
        max and ``bits`` (default ``53 - ceil(log2(n_total))``).  Returns the ``(ll_max, bits)`` used, the same on every rank.
        ``reference`` (``Ensemble.loglik``): the observations of those variables are anomalies from a reference period, so an
        anomaly plume (``quantile_rows_global(..., weighted=True, anomaly=True)``) is weighted by anomaly fit."""
        ll = self.ensemble.loglik(obs_var, obs_tidx, obs_value, obs_sigma, normalize, on_device=True, reference=reference)
        return self.constrain_loglik(ll, bits)

    def constrain_loglik(self, ll, bits: Optional[int] = None):
        """``constrain`` from a per-member log-likelihood of this rank's members (numpy or a ``DeviceVector``), e.g.
        ``ensemble.loglik_vectors(...)`` over variability statistics or ``ensemble.loglik_spectrum(...)`` over the band powers of
        ``ensemble.spectrum(...)``, alone or added onto a point likelihood: the local max, a MAX all-reduce,
        ``set_weights_from_loglik``.  Both statistics are per member -- a shard's vectors are the whole ensemble's, cut -- so the
        sharded ensemble needs no entry point of its own for them.  Returns the ``(ll_max, bits)`` used, the same on every rank."""
        from .ensemble import default_weight_bits
        ll_max = self.ensemble.loglik_max(ll)
        if is_distributed():
            import torch
            d = _dist()
            m = torch.tensor([ll_max], dtype=torch.float64, device=_device_for_backend())
            d.all_reduce(m, op=d.ReduceOp.MAX)
            ll_max = float(m.item())
        if bits is None:
            bits = default_weight_bits(self.n_total)
        return self.ensemble.set_weights_from_loglik(ll, bits, ll_max)

    def weights_stats_global(self) -> Dict[str, object]:
        """Exact weight statistics and effective sample size of the global ensemble (``weights_stats_global``)."""
        return weights_stats_global(self.ensemble)

    def resample(self, n_draws: int, seed: int = 0, offset: Optional[int] = None):
        """This rank's ``(k_first, count, ancestors)`` of one systematic draw from the global ensemble (``resample_global``)."""
        return resample_global(self.ensemble, n_draws, seed, offset=offset)
