"""A recording stand-in for the library side of ``ModelBuilder.build()`` on the graph path: with ``recording()`` active,
``rscm_amd.core.Ensemble`` is a class that takes ``var_ids`` and ``input_rows`` from ``L.KIND_TABLE`` and logs its constructor
arguments and every method call, and ``L.load()`` returns a stub with the three library functions the builder calls itself
(stream create / destroy, ``rscm_ens_set_link_order_check``).  The whole graph build then runs with no library and no device, and
``Recorder.log`` is the transcript of what it would have asked the library to do: ensembles appear as their creation index,
small arrays whole, large ones as shape plus a SHA-256 of their float64 bytes, NaN as the string "nan".  ``snapshot`` is the
same encoding of the ``GraphModel`` attributes that tests and ``rscm_amd/serialise.py`` read.  No product code beyond the tables."""
import contextlib
import hashlib
import math

import numpy as np

from rscm_amd import _lib as L
from rscm_amd import core

SMALL = 16   # arrays of up to this many values are logged whole


def enc(x):
    """JSON-ready and comparable with ``==``: floats that JSON or ``==`` cannot carry as strings, arrays by size."""
    if isinstance(x, RecordingEnsemble):
        return {"ensemble": x.index}
    if isinstance(x, (bool, str)) or x is None:
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        x = float(x)
        return x if math.isfinite(x) else repr(x)
    if isinstance(x, dict):
        return [[enc(k), enc(v)] for k, v in x.items()]   # a list of pairs: the order is part of the record
    if isinstance(x, (list, tuple)) and not all(isinstance(v, (int, float, np.number)) and not isinstance(v, bool) for v in x):
        return [enc(v) for v in x]
    a = np.asarray(x, dtype=np.float64)
    if a.size <= SMALL:
        return {"shape": list(a.shape), "values": [enc(v) for v in a.reshape(-1)]}
    return {"shape": list(a.shape), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}


def enc_members(a, axis):
    """An array with a member axis: where every member holds the same values, those once and the member count beside them, so that
    two transcripts that differ in ``n_members`` alone differ in these counts alone."""
    a = np.asarray(a, dtype=np.float64)
    first = np.take(a, [0], axis=axis)
    if a.shape[axis] and np.array_equal(np.broadcast_to(first, a.shape), a, equal_nan=True):
        return {"members": a.shape[axis], "each": enc(np.take(a, 0, axis=axis))}
    return enc(a)


class Recorder:
    def __init__(self):
        self.log = []
        self.ensembles = []

    def add(self, *entry):
        self.log.append([enc(v) for v in entry])

    # -- the library functions the builder and GraphModel.close call directly
    def rscm_gpu_stream_create(self, device, ref):
        self.add("rscm_gpu_stream_create", device)
        return L.OK

    def rscm_gpu_stream_destroy(self, device, stream):
        self.add("rscm_gpu_stream_destroy", device)
        return L.OK

    def rscm_ens_set_link_order_check(self, h, enabled):
        self.add("rscm_ens_set_link_order_check", self.ensembles[h - 1], enabled)
        return L.OK


_active = None


class RecordingEnsemble:
    """``rscm_amd.ensemble.Ensemble`` as far as the graph build uses it (same constructor signature and defaults)."""

    def __init__(self, kind, n_members, time_bounds, device=0, store_series=True, window_rows=None, output_stride=0,
                 output_vars=None, forcing_components=None, noise_params=False):
        rec = self._rec = _active
        rec.ensembles.append(self)
        self.index = len(rec.ensembles) - 1
        self._h = self.index + 1   # what Ensemble keeps its handle in: truthy until close()
        self.kind, self.n_members, self.device = kind, int(n_members), device
        self.bounds = np.asarray(time_bounds, dtype=np.float64)
        self.n_times = len(self.bounds) - 1
        var_ids, self.n_params, self.input_rows = L.KIND_TABLE[kind]
        self.var_ids = dict(var_ids)
        self._params = None
        rec.add("Ensemble", self.index, {"kind": kind, "n_members": self.n_members, "time_bounds": self.bounds, "device": device,
                                        "store_series": store_series, "window_rows": window_rows, "output_stride": output_stride,
                                        "output_vars": None if output_vars is None else [int(v) for v in output_vars],
                                        "forcing_components": forcing_components, "noise_params": noise_params})

    def set_stream(self, hip_stream):
        self._rec.add("set_stream", self)

    def set_params(self, soa):
        self._params = np.array(soa, dtype=np.float64)
        assert self._params.shape == (self.n_params, self.n_members), (self._params.shape, self.n_params, self.n_members)
        self._rec.add("set_params", self, enc_members(self._params, 1))

    def get_params(self):
        return self._params.copy()

    def set_step_size(self, component, step):
        self._rec.add("set_step_size", self, component, step)

    def link_input(self, input_row, src, src_var, source=L.SRC_EXOGENOUS):
        self._rec.add("link_input", self, input_row, src, src_var, source)

    def unlink_input(self, input_row):
        self._rec.add("unlink_input", self, input_row)

    def set_forcing(self, series, scenario_of_member=None, source=L.SRC_EXOGENOUS, member_offset=0):
        self._rec.add("set_forcing", self, np.asarray(series, dtype=np.float64), scenario_of_member, source)

    def set_initial(self, var, values):
        self._rec.add("set_initial", self, var, enc_members(np.broadcast_to(np.asarray(values, dtype=np.float64), (self.n_members,)), 0))

    def close(self):
        if self._h:
            self._rec.add("close", self)
            self._h = None


@contextlib.contextmanager
def recording():
    """``core.Ensemble`` and ``L.load`` replaced for the duration; yields the ``Recorder``."""
    global _active
    rec = Recorder()
    saved = (core.Ensemble, L.load, _active)
    core.Ensemble, L.load, _active = RecordingEnsemble, (lambda: rec), rec
    try:
        yield rec
    finally:
        core.Ensemble, L.load, _active = saved


MODEL_ATTRIBUTES = ("_order", "_var_home", "_links", "_feed_forward", "_reads_unwritten", "_fourbox", "_fourbox_aggregates", "_windowed",
                    "_output_stride", "_exogenous", "_sources", "param_home", "base_params", "_execution_order")


def snapshot(model, builder=None):
    """The ``GraphModel`` attributes that tests and ``serialise`` read, encoded like the transcript; dicts keep their order."""
    out = {name: enc(getattr(model, name)) for name in MODEL_ATTRIBUTES}
    out["ensembles"] = [[name, ens.index] for name, ens in model.ensembles.items()]
    out["_host_nodes"] = [[name, {"component": node.comp.type_name, "sources": enc(node.sources), "device_reads": enc(node.device_reads),
                                  "series": [[v, enc_members(s, 1)] for v, s in node.series.items()]}]
                          for name, node in model._host_nodes.items()]
    out["_builder"] = model._builder is builder if builder is not None else model._builder is not None
    return out
