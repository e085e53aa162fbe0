"""``Ensemble``: one device-resident batch of model instances behind the C-ABI.

This is the host-side object the reference-shaped front-ends (``rscm_amd.core.Model``,
``rscm_amd.calibrate.ModelRunner``) drive.  It owns one ``rscm_ens`` handle = one GPU; all
arithmetic happens in the HIP kernels.  Semantics follow the reference's stepper
(crates/rscm-core/src/model/runtime.rs:504-527): ``step()`` solves the current step and writes
index ``time_index + 1``; ``run()`` steps to the end of the axis.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


class DeviceVector:
    """A per-member vector left in device memory by an ensemble (``loglik(..., on_device=True)``,
    ``status_device()``): owned by the handle and valid until its next call of the same kind.  It
    carries ``__cuda_array_interface__``, so ``torch.as_tensor(v, device="cuda")`` is a zero-copy
    view -- what the RCCL all-gather of ``rscm_amd.distributed`` sends -- and ``to_host()`` copies it
    out through the library."""

    def __init__(self, ptr: int, n: int, dtype, owner: "Ensemble"):
        self.ptr, self.n, self.dtype, self.owner = int(ptr), int(n), np.dtype(dtype), owner

    def __len__(self) -> int:
        return self.n

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.n,), "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2,
                "strides": None}

    def to_host(self) -> np.ndarray:
        out = np.empty(self.n, dtype=self.dtype)
        L.check(L.load().rscm_gpu_copy_to_host(self.owner.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                               out.nbytes))
        return out


class Ensemble:
    def __init__(self, kind: int, n_members: int, time_bounds: Sequence[float], device: int = 0,
                 store_series: bool = True, window_rows: Optional[int] = None, output_stride: int = 0,
                 output_vars: Optional[Sequence] = None, forcing_components=None, noise_params: bool = False):
        """``window_rows``: keep only a sliding window of that many rows of every series
        (``RSCM_FLAG_WINDOWED``) plus, with ``output_stride`` > 0, every ``output_stride``-th row of
        ``output_vars`` (names or ids; None: all) -- for long axes stepped in lock-step.

        ``forcing_components`` (two-layer kind; an int K or a sequence of K names, 1 <= K <= 8): a *mix*
        ensemble (``rscm_ens_create_mix``).  ``set_forcing`` then takes K component series per scenario,
        ``[S][K][T]``, and member i is forced by ``((S_0 c_0 + S_1 c_1) + ...) + S_K-1 c_K-1`` with its own
        coefficients c_k = parameter rows 6 .. 6+K-1 (``coefficient_row``): ``n_params`` is 6 + K.

        ``noise_params`` (two-layer kind, plain or mix, whole series stored): two more parameter rows after the coefficients
        (``RSCM_FLAG_NOISE_PARAMS``), every member's noise amplitude and persistence (``noise_param_rows``,
        ``set_forcing_noise_members``): ``n_params`` is 6 + K + 2."""
        self._lib = L.load()
        b = L.f64(time_bounds)
        if b.ndim != 1 or len(b) < 3:
            raise ValueError("time_bounds needs at least 3 entries (2 time points)")
        self.kind = kind
        self.n_members = int(n_members)
        self.n_times = len(b) - 1
        self.bounds = b
        self.device = device
        var_ids, self.n_params, input_rows = L.KIND_TABLE[kind]
        self.n_forcing_components = 0
        if forcing_components is not None:
            if kind != L.KIND_TWO_LAYER:
                raise ValueError("forcing_components are available for the two-layer kind only")
            if window_rows is not None:
                raise ValueError("a mix ensemble has no windowed storage")
            names = (tuple(f"component_{k}" for k in range(forcing_components)) if isinstance(forcing_components, (int, np.integer))
                     else tuple(str(x) for x in forcing_components))
            if not 1 <= len(names) <= L.TL_MAX_COMPONENTS or len(set(names)) != len(names):
                raise ValueError(f"forcing_components: 1 to {L.TL_MAX_COMPONENTS} distinct components, got {len(names)} name(s)")
            self.n_forcing_components = len(names)
            self.n_params = L.TL_P_COEFF0 + len(names)   # the coefficients are parameter rows 6 .. 6 + K - 1
            input_rows = names
        self.noise_params = bool(noise_params)
        if self.noise_params:
            if kind != L.KIND_TWO_LAYER:
                raise ValueError("noise_params are available for the two-layer kind only")
            if window_rows is not None or not store_series:
                raise ValueError("noise_params need an ensemble that stores its whole series (no window_rows, store_series=True)")
            self.n_params += 2   # sigma_i and phi_i follow the six parameters and the coefficients
        flag = L.FLAG_NOISE_PARAMS if self.noise_params else 0
        self.var_ids: Dict[str, int] = dict(var_ids)
        self.n_vars = max(self.var_ids.values()) + 1   # the stored variables and the input; diagnostics get the ids from here on
        self._diagnostic_names: Dict[str, int] = {}    # the names define_diagnostic added to var_ids
        self.input_rows = input_rows  # names of the rows of the input block, or None
        self.n_inputs = len(input_rows) if input_rows else 1
        h = C.c_void_p()
        self.store_series = bool(store_series)
        self.window_rows = None if window_rows is None or window_rows >= self.n_times else int(window_rows)
        self.output_stride = int(output_stride) if self.window_rows else 0
        if self.n_forcing_components:
            L.check(self._lib.rscm_ens_create_mix(kind, self.n_members, self.n_times, L.dptr(b), device,
                                                  flag if store_series else L.FLAG_NO_SERIES, self.n_forcing_components, C.byref(h)))
        elif self.window_rows:
            ov = None
            if output_vars is not None:
                ov = np.ascontiguousarray([self._var(v) for v in output_vars], dtype=np.int32)
            self.output_vars = None if ov is None else [int(v) for v in ov]
            L.check(self._lib.rscm_ens_create_windowed(kind, self.n_members, self.n_times, L.dptr(b), device, L.FLAG_WINDOWED,
                                                       self.window_rows, self.output_stride, -1 if ov is None else len(ov),
                                                       L.iptr(ov), C.byref(h)))
        else:
            L.check(self._lib.rscm_ens_create_ex(kind, self.n_members, self.n_times, L.dptr(b), device,
                                                 flag if store_series else L.FLAG_NO_SERIES, C.byref(h)))
        self._h = h
        # the library and the tables of this package must agree on the shape of the kind
        got = [C.c_int32() for _ in range(3)]
        for fn, x in zip((self._lib.rscm_ens_n_params, self._lib.rscm_ens_n_vars, self._lib.rscm_ens_n_inputs), got):
            L.check(fn(self._h, C.byref(x)))
        want = (self.n_params, max(self.var_ids.values()) + 1, self.n_inputs)   # (a mix ensemble: 6 + K rows, K inputs)
        if tuple(x.value for x in got) != want:
            self.close()
            raise RuntimeError(f"kind {kind}: library reports (params, vars, inputs) = {tuple(x.value for x in got)}, "
                               f"package tables say {want}")
        k = C.c_int32()
        L.check(self._lib.rscm_ens_n_forcing_components(self._h, C.byref(k)))
        if k.value != self.n_forcing_components:
            self.close()
            raise RuntimeError(f"library reports {k.value} forcing components, asked for {self.n_forcing_components}")

    # -- lifecycle --------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            L.check(self._lib.rscm_ens_destroy(self._h))  # fails while other ensembles link to this one
            self._h = None
            self._linked = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _var(self, var) -> int:
        return self.var_ids[var] if isinstance(var, str) else int(var)

    # -- configuration ----------------------------------------------------------------------
    def set_mode(self, mode: int) -> None:
        L.check(self._lib.rscm_ens_set_mode(self._h, mode))

    def set_step_size(self, component: int, step: float) -> None:
        L.check(self._lib.rscm_ens_set_step_size(self._h, component, float(step)))

    def set_params(self, soa) -> None:
        p = L.f64(soa)
        if p.shape != (self.n_params, self.n_members):
            raise ValueError(f"params must be [{self.n_params}][{self.n_members}], got {p.shape}")
        L.check(self._lib.rscm_ens_set_params(self._h, L.dptr(p)))

    def set_params_aos(self, aos) -> None:
        p = L.f64(aos)
        if p.shape != (self.n_members, self.n_params):
            # mirrors model_runner.rs:225-231 "Expected {} parameters, got {}"
            raise ValueError(f"Expected {self.n_params} parameters per member "
                             f"([{self.n_members}][{self.n_params}]), got {p.shape}")
        L.check(self._lib.rscm_ens_set_params_aos(self._h, L.dptr(p)))

    def coefficient_row(self, component) -> int:
        """The parameter row that holds the coefficient of a forcing component (name or index) of a mix ensemble."""
        if not self.n_forcing_components:
            raise ValueError("not a mix ensemble (forcing_components was not given)")
        k = self.input_rows.index(component) if isinstance(component, str) else int(component)
        if not 0 <= k < self.n_forcing_components:
            raise ValueError(f"component {component!r} out of range [0, {self.n_forcing_components})")
        return L.TL_P_COEFF0 + k

    def set_forcing(self, series, scenario_of_member=None, source: int = L.SRC_EXOGENOUS,
                    var=0) -> None:
        s = L.f64(series)
        if self.input_rows:  # a block of rows per scenario: [S][n_inputs][T] or [n_inputs][T]
            if s.ndim == 1 and self.n_inputs == 1:
                s = s[None, None]
            elif s.ndim == 2:
                # one input row: [S][T]; several: one scenario's [n_inputs][T]
                s = s[:, None] if self.n_inputs == 1 else s[None]
            if s.ndim != 3 or s.shape[1:] != (self.n_inputs, self.n_times):
                raise ValueError(f"input block must be [S][{self.n_inputs}][{self.n_times}], got {s.shape}")
            s = np.ascontiguousarray(s)
        else:
            s = np.atleast_2d(s)
            if s.shape[1] != self.n_times:
                raise ValueError(f"forcing must have {self.n_times} time points, got {s.shape[1]}")
        sc = None
        if scenario_of_member is not None:
            sc = np.ascontiguousarray(scenario_of_member, dtype=np.int32)
            if sc.shape != (self.n_members,):
                raise ValueError("scenario_of_member must have one entry per member")
        L.check(self._lib.rscm_ens_set_forcing(self._h, self._var(var), s.shape[0], L.dptr(s),
                                               L.iptr(sc), source))

    def set_forcing_noise(self, sigma: float, seed: int, member_offset: int = 0, phi: float = 0.0) -> None:
        """Internal variability (two-layer kind, mix ensembles included): member i is forced at forcing-axis index t by
        ``F + sigma * z(seed, member_offset + i, t)``, z a standard normal deviate that is a pure function of its three
        arguments (``rscm_ens_set_forcing_noise``) -- white in t, independent between members, the same whatever way the run is
        cut, rewound, checkpointed or branched.  ``member_offset`` is the global index of this ensemble's first member (a shard
        passes its own).  The fused ``run_loglik``, ``link_input``, ``run_lockstep`` and the device sampler refuse such an
        ensemble; ``run()`` followed by ``loglik()`` scores it.

        ``phi != 0`` (``|phi| < 1``) makes the noise red (``rscm_ens_set_forcing_noise_ar1``): ``F + e_t`` with
        ``e_0 = sigma * z_0`` and ``e_t = phi * e_{t-1} + sigma * sqrt(1 - phi**2) * z_t``, variance ``sigma**2`` at every index
        and lag-one correlation ``phi`` per forcing-axis index.  e is as pure a function as z; the ensemble caches each member's
        value at the last index it ran (``forcing_noise_cached_index``) and forms it again from the draws wherever a run starts
        elsewhere.  ``phi=0.0`` is the white setting, bit for bit."""
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must fit 64 unsigned bits, got {seed}")
        L.check(self._lib.rscm_ens_set_forcing_noise_ar1(self._h, C.c_uint64(seed), float(sigma), float(phi), int(member_offset)))

    @property
    def noise_param_rows(self):
        """``(sigma_row, phi_row)``: the parameter rows that hold every member's noise amplitude and persistence
        (``noise_params=True``; 6 + K and 6 + K + 1)."""
        s, p = C.c_int32(), C.c_int32()
        L.check(self._lib.rscm_ens_forcing_noise_members(self._h, None, C.byref(s), C.byref(p)))
        if s.value < 0:
            raise ValueError("this ensemble has no noise parameter rows (noise_params=True was not given)")
        return s.value, p.value

    def set_forcing_noise_members(self, seed: int, member_offset: int = 0) -> None:
        """Internal variability with every member's own amplitude and persistence (``rscm_ens_set_forcing_noise_members``; an
        ensemble made with ``noise_params=True``): member i is forced by ``F + e_t``, the red recurrence of ``set_forcing_noise``
        with ``sigma_i`` and ``phi_i`` from the rows ``noise_param_rows`` as they stand when a run is launched.  The rows are
        parameters like any other: ``sample_lhs`` draws them, ``set_weights_from_loglik`` weights them, ``params_vector`` with
        ``quantile_vectors(..., weighted=True)`` reports their posterior, ``posterior()`` / ``branch()`` hand them to the draws.
        Nothing validates them: a NaN or Inf row, or ``|phi_i| > 1``, gives that member NaN states and a failed status, nothing
        else.  Everything that writes a parameter row drops the cached values (``forcing_noise_cached_index``); once
        ``params_devptr`` has been taken every run forms them again."""
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must fit 64 unsigned bits, got {seed}")
        L.check(self._lib.rscm_ens_set_forcing_noise_members(self._h, C.c_uint64(seed), int(member_offset)))

    def clear_forcing_noise(self) -> None:
        L.check(self._lib.rscm_ens_clear_forcing_noise(self._h))

    @property
    def forcing_noise(self) -> Optional[Dict[str, object]]:
        """``{"sigma", "seed", "member_offset"}`` of ``set_forcing_noise``, and ``"phi"`` where the noise is red (``phi != 0``);
        ``{"per_member": True, "seed", "member_offset"}`` under ``set_forcing_noise_members``; None without noise."""
        on, seed, sigma, off, phi, per = C.c_int32(), C.c_uint64(), C.c_double(), C.c_int64(), C.c_double(), C.c_int32()
        L.check(self._lib.rscm_ens_forcing_noise(self._h, C.byref(on), C.byref(seed), C.byref(sigma), C.byref(off)))
        if not on.value:
            return None
        L.check(self._lib.rscm_ens_forcing_noise_members(self._h, C.byref(per), None, None))
        if per.value:
            return {"per_member": True, "seed": seed.value, "member_offset": off.value}
        L.check(self._lib.rscm_ens_forcing_noise_ar1(self._h, C.byref(phi), None))
        noise = {"sigma": sigma.value, "seed": seed.value, "member_offset": off.value}
        if phi.value != 0.0:
            noise["phi"] = phi.value
        return noise

    @property
    def forcing_noise_cached_index(self) -> int:
        """The forcing-axis index at which the red noise's per-member values are cached, -1 when nothing is (white or no noise,
        after any setter of the noise, before the first run): a run that starts right after it loads them, any other forms them
        again from the draws."""
        at = C.c_int32()
        L.check(self._lib.rscm_ens_forcing_noise_ar1(self._h, None, C.byref(at)))
        return at.value

    def forcing_noise_rows(self, t_begin: int = 0, t_end: Optional[int] = None) -> np.ndarray:
        """``[t_end - t_begin][N]``: the term the members' forcing gets at forcing-axis indices ``t_begin .. t_end - 1``: ``sigma * z``,
        or ``e`` of the red noise."""
        t_end = self.n_times if t_end is None else int(t_end)
        out = np.empty((max(t_end - int(t_begin), 0), self.n_members))
        L.check(self._lib.rscm_ens_forcing_noise_rows(self._h, int(t_begin), t_end, L.dptr(out), 0))
        return out

    def link_input(self, input_row, src: "Ensemble", src_var, source: int = L.SRC_EXOGENOUS) -> None:
        """Read input row ``input_row`` (index or name) member by member from ``src``'s stored
        series ``src_var`` instead of the scenario table: an edge of a component graph kept on the
        device.  ``source`` is this consumer's VariableSource (``SRC_EXOGENOUS``: index n,
        ``SRC_UPSTREAM``: n+1).  Both ensembles must share a stream; ``src`` must outlive the link."""
        row = (self.input_rows.index(input_row) if self.input_rows else 0) if isinstance(input_row, str) else int(input_row)
        L.check(self._lib.rscm_ens_link_input(self._h, row, src._h, src._var(src_var), source))
        self._linked = getattr(self, "_linked", {})
        self._linked[row] = src  # keeps the producer alive as long as this consumer

    def unlink_input(self, input_row) -> None:
        row = (self.input_rows.index(input_row) if self.input_rows else 0) if isinstance(input_row, str) else int(input_row)
        L.check(self._lib.rscm_ens_unlink_input(self._h, row))
        getattr(self, "_linked", {}).pop(row, None)

    def set_initial(self, var, values) -> None:
        v = np.atleast_1d(L.f64(values))
        L.check(self._lib.rscm_ens_set_initial(self._h, self._var(var), L.dptr(v), v.size))

    def set_state(self, var, time_index: int, values) -> None:
        """Overwrite row ``time_index`` of a stored series (1 value = broadcast, or one per member)."""
        v = np.atleast_1d(L.f64(values))
        L.check(self._lib.rscm_ens_set_state(self._h, self._var(var), int(time_index), L.dptr(v), v.size))

    def set_time_index(self, time_index: int) -> None:
        L.check(self._lib.rscm_ens_set_time_index(self._h, int(time_index)))

    def set_stream(self, hip_stream: Optional[int]) -> None:
        L.check(self._lib.rscm_ens_set_stream(self._h, C.c_void_p(hip_stream)))

    def sample_lhs(self, seed: int, low, high, member_offset: int = 0,
                   n_total: Optional[int] = None) -> None:
        lo, hi = L.f64(low), L.f64(high)
        if lo.shape != (self.n_params,) or hi.shape != (self.n_params,):
            raise ValueError("low/high need one entry per parameter")
        n_total = self.n_members if n_total is None else n_total
        L.check(self._lib.rscm_ens_sample_lhs(self._h, C.c_uint64(seed), L.dptr(lo), L.dptr(hi),
                                              member_offset, n_total))

    def sample_lhs_priors(self, seed: int, priors, base=None, member_offset: int = 0, n_total: Optional[int] = None) -> None:
        """The Latin hypercube of ``sample_lhs`` -- the same strata for the same seed -- through each row's own inverse CDF on the
        device (``rscm_ens_sample_lhs_priors``).  ``priors``: ``{row: distribution}`` of ``calibrate.Uniform`` / ``Normal`` /
        ``LogNormal`` or a ``Bound`` of one (``ParameterSet.rows`` makes it from a named set); the rows it leaves out stay fixed at
        ``base[row]``.  A block of a larger ensemble takes ``member_offset`` and ``n_total`` as ``sample_lhs`` does."""
        from .calibrate import prior_table
        kind, a, b, p0, p1, lo, hi = prior_table(priors, self.n_params, base)
        n_total = self.n_members if n_total is None else n_total
        L.check(self._lib.rscm_ens_sample_lhs_priors(self._h, C.c_uint64(seed), L.iptr(kind), L.dptr(a), L.dptr(b), L.dptr(p0),
                                                     L.dptr(p1), L.dptr(lo), L.dptr(hi), member_offset, n_total))

    def get_params(self) -> np.ndarray:
        out = np.empty((self.n_params, self.n_members))
        L.check(self._lib.rscm_ens_get_params(self._h, L.dptr(out)))
        return out

    # -- stepping ---------------------------------------------------------------------------
    @property
    def time_index(self) -> int:
        n = C.c_int32()
        L.check(self._lib.rscm_ens_time_index(self._h, C.byref(n)))
        return n.value

    def step(self) -> None:
        n = self.time_index
        L.check(self._lib.rscm_ens_run(self._h, n, n + 1))

    def run(self, step_end: Optional[int] = None, *, sync: bool = True) -> None:
        end = self.n_times - 1 if step_end is None else step_end
        fn = self._lib.rscm_ens_run if sync else self._lib.rscm_ens_run_async
        L.check(fn(self._h, self.time_index, end))

    def sync(self) -> None:
        L.check(self._lib.rscm_ens_sync(self._h))

    def rewind(self) -> None:
        L.check(self._lib.rscm_ens_rewind(self._h))

    def clear_series(self) -> None:
        """Rewind and make every stored row after index 0 NaN again (a fresh collection)."""
        L.check(self._lib.rscm_ens_clear_series(self._h))

    def finished(self) -> bool:
        return self.time_index == self.n_times - 1

    def last_run_ms(self) -> float:
        ms = C.c_float()
        L.check(self._lib.rscm_ens_last_run_ms(self._h, C.byref(ms)))
        return ms.value

    def last_run_plan(self):
        """(member blocks, step chunks) the most recent run was cut into: (2, k) when a whole-axis run of the two-layer or the
        coupled kind -- or an unlinked ClimateUDEB run over more than 65 536 members (two halves, each chunk reloading and storing
        the block's columns) -- was issued as two member blocks on two streams in k chunks of model steps
        (rscm_ens_last_run_plan), else (1, 1)."""
        mb, sc = C.c_int32(), C.c_int32()
        L.check(self._lib.rscm_ens_last_run_plan(self._h, C.byref(mb), C.byref(sc)))
        return mb.value, sc.value

    # -- checkpoint / resume ------------------------------------------------------------------
    def state_vars(self) -> Dict[str, int]:
        """The State variables of the kind (what the stepper reads back at the next step)."""
        ids = {L.KIND_TWO_LAYER: (1, 2), L.KIND_COUPLED: (1, 5), L.KIND_UDEB: (1, 4), L.KIND_CH4_CHEMISTRY: (1, 1),
               L.KIND_N2O_CHEMISTRY: (1, 1), L.KIND_CO2_BUDGET: (1, 1), L.KIND_TERRESTRIAL_CARBON: (1, 4),
               L.KIND_OCEAN_CARBON: (1, 2), L.KIND_HALOCARBON: (1, len(L.HC_SPECIES)), L.KIND_CARBON_CYCLE: (1, 3)}
        lo, hi = ids.get(self.kind, (1, 0))  # the other kinds are stateless
        return {k: v for k, v in self.var_ids.items() if lo <= v <= hi}

    def _history_depth(self) -> int:
        """Rows before the current one that the next step reads (previous() / at_offset(-k))."""
        if self.kind == L.KIND_CH4_CHEMISTRY:
            return 1
        if self.kind == L.KIND_N2O_CHEMISTRY:  # at_offset(-(strat_delay + 1)), n2o.rs:203-218
            return int(max(1.0, np.nanmax(self.get_params()[L.N2O_PARAM_NAMES.index("strat_delay")]))) + 1
        return 0

    def checkpoint(self, all_variables: bool = False) -> Dict[str, object]:
        """What is needed to resume: time index, parameters, row ``time_index`` of every state
        variable (``all_variables``: of every stored variable -- what linked consumers read), the
        earlier rows the chemistry kinds look back at, and the internal component state of
        ClimateUDEB / OceanCarbon.  The reference's checkpoint holds time_index, the whole collection
        and the component states (crates/rscm-core/src/model/runtime.rs:270-282)."""
        k = self.time_index
        names = {n: v for n, v in self.var_ids.items() if 0 < v < self.n_vars} if all_variables else self.state_vars()   # (no diagnostics)
        depth = min(self._history_depth(), k)
        history = {name: self.get_series(v, k - depth, k) for name, v in self.state_vars().items()} if depth else {}
        n = C.c_int64()
        L.check(self._lib.rscm_ens_internal_state_size(self._h, C.byref(n)))
        internal = None
        if n.value:
            internal = np.empty(n.value)
            L.check(self._lib.rscm_ens_get_internal_state(self._h, L.dptr(internal)))
        ck = {"kind": self.kind, "n_members": self.n_members, "bounds": self.bounds.copy(),
              "time_index": k, "params": self.get_params(),
              "state": {name: self.get_series(v, k, k + 1)[0] for name, v in names.items()},
              "history": history, "internal": internal}
        noise = self.forcing_noise if self.kind == L.KIND_TWO_LAYER else None
        if noise is not None and noise.get("per_member"):   # (sigma_i and phi_i are in the parameter block already)
            ck["forcing_noise"] = {"per_member": True, "seed": np.uint64(noise["seed"]), "member_offset": noise["member_offset"]}
        elif noise is not None:   # (a pure function of these numbers: the red noise's cached values are not carried)
            ck["forcing_noise"] = {"sigma": noise["sigma"], "seed": np.uint64(noise["seed"]), "member_offset": noise["member_offset"]}
            if "phi" in noise:
                ck["forcing_noise"]["phi"] = noise["phi"]
        return ck

    def restore(self, ck: Dict[str, object], clear_later_rows: bool = False) -> None:
        """``clear_later_rows``: make every stored row after the checkpoint's time index NaN again, as
        in the collection the checkpoint was taken from -- needed when an already advanced ensemble is
        rolled back and a linked consumer reads rows its producer has not rewritten yet."""
        if (ck["kind"] != self.kind or ck["n_members"] != self.n_members
                or not np.array_equal(ck["bounds"], self.bounds)):
            raise ValueError("checkpoint does not match this ensemble (kind, members or time axis)")
        per_member = bool((ck.get("forcing_noise") or {}).get("per_member", False))
        if per_member and not self.noise_params:
            raise ValueError("the checkpoint carries per-member forcing noise: restore it into an ensemble made with noise_params=True")
        self.set_params(ck["params"])
        if self.kind == L.KIND_TWO_LAYER:   # the noise setting is the checkpoint's: none where it has none
            noise = ck.get("forcing_noise")
            if noise is None:
                self.clear_forcing_noise()
            elif per_member:
                self.set_forcing_noise_members(int(noise["seed"]), int(noise["member_offset"]))
            else:
                self.set_forcing_noise(float(noise["sigma"]), int(noise["seed"]), int(noise["member_offset"]), float(noise.get("phi", 0.0)))
        k = int(ck["time_index"])
        # the stepper first: a windowed ensemble positions its window at k, then the rows go in
        internal = ck.get("internal")
        if internal is not None:
            blob = L.f64(internal)
            L.check(self._lib.rscm_ens_set_internal_state(self._h, L.dptr(blob), blob.size, k))
        else:
            L.check(self._lib.rscm_ens_set_time_index(self._h, k))
        for name, row in ck["state"].items():
            self.set_state(name, k, row)
        for name, rows in ck.get("history", {}).items():
            for d, row in enumerate(rows):
                self.set_state(name, k - len(rows) + d, row)
        if clear_later_rows and self.store_series and not self.window_rows:
            L.check(self._lib.rscm_ens_clear_rows_after(self._h, k))

    # -- outputs ----------------------------------------------------------------------------
    def get_series(self, var, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                   m_begin: int = 0, m_end: Optional[int] = None,
                   out: Optional[np.ndarray] = None) -> np.ndarray:
        """``[n_t][m_end - m_begin]`` copy of a stored series.  Pass ``out`` (e.g. from
        ``pinned_empty``) to reuse a buffer; a page-locked one is filled by DMA at PCIe rate."""
        t_end = self.n_times if t_end is None else t_end
        m_end = self.n_members if m_end is None else m_end
        nt = len(range(t_begin, t_end, t_stride))
        if out is None:
            out = np.empty((nt, m_end - m_begin))
        elif out.shape != (nt, m_end - m_begin) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float64 array of shape {(nt, m_end - m_begin)}")
        L.check(self._lib.rscm_ens_get_series(self._h, self._var(var), t_begin, t_end, t_stride,
                                              m_begin, m_end, L.dptr(out)))
        return out

    def series_devptr(self, var) -> int:
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_series_devptr(self._h, self._var(var), C.byref(p)))
        return p.value

    def status(self) -> np.ndarray:
        out = np.empty(self.n_members, dtype=np.uint8)
        L.check(self._lib.rscm_ens_status(self._h, L.bptr(out)))
        return out

    def status_device(self) -> DeviceVector:
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_status_devptr(self._h, C.byref(p)))
        self.sync()
        return DeviceVector(p.value, self.n_members, np.uint8, self)

    def _reference(self, reference):
        """``{variable: (t_begin, t_end[, t_stride])}`` in row indices (the rows of ``set_baseline``) as the C boundary's arrays."""
        rv, rb, re_, rs = [], [], [], []
        for var, rows in dict(reference).items():
            rows = tuple(int(x) for x in rows)
            if len(rows) not in (2, 3):
                raise ValueError(f"reference period of {var!r}: (t_begin, t_end[, t_stride]) expected, got {rows}")
            rv.append(self._var(var)), rb.append(rows[0]), re_.append(rows[1]), rs.append(rows[2] if len(rows) == 3 else 1)
        return tuple(np.ascontiguousarray(x, dtype=np.int32) for x in (rv, rb, re_, rs))

    def _loglik(self, entry, obs_var, obs_tidx, obs_value, obs_sigma, normalize, on_device, reference):
        """``entry`` is ``"loglik"`` or ``"run_loglik"``: calls ``rscm_ens_{entry}[_ref][_device]``."""
        ov = np.ascontiguousarray([self._var(v) for v in np.atleast_1d(obs_var)], dtype=np.int32)
        ot = np.ascontiguousarray(obs_tidx, dtype=np.int32)
        val, sig = L.f64(obs_value), L.f64(obs_sigma)
        if not (len(ov) == len(ot) == len(val) == len(sig)):
            raise ValueError("observation arrays differ in length")
        args = [self._h, len(ov), L.iptr(ov), L.iptr(ot), L.dptr(val), L.dptr(sig), int(normalize)]
        if reference:
            ref = self._reference(reference)
            args += [len(ref[0])] + [L.iptr(x) for x in ref]
        fn = getattr(self._lib, "rscm_ens_" + entry + ("_ref" if reference else "") + ("_device" if on_device else ""))
        if on_device:
            p = C.c_void_p()
            L.check(fn(*args, C.byref(p)))
            return DeviceVector(p.value, self.n_members, np.float64, self)
        out = np.empty(self.n_members)
        L.check(fn(*args, L.dptr(out)))
        return out

    def loglik(self, obs_var, obs_tidx, obs_value, obs_sigma, normalize: bool = False, on_device: bool = False, reference=None):
        """Gaussian log-likelihood per member, ``[N]``; ``on_device`` leaves it in device memory (a
        ``DeviceVector``) for a reduction or all-gather without a host round trip.  ``reference``:
        ``{variable: (t_begin, t_end[, t_stride])}`` in row indices -- that variable's observations are anomalies from the
        member's own mean over those rows (rscm_ens_loglik_ref)."""
        return self._loglik("loglik", obs_var, obs_tidx, obs_value, obs_sigma, normalize, on_device, reference)

    def run_loglik(self, obs_var, obs_tidx, obs_value, obs_sigma, normalize: bool = False, on_device: bool = False, reference=None):
        """Fused run + Gaussian log-likelihood: no series is written (see rscm_ens_run_loglik).  ``reference`` as for ``loglik``
        (rscm_ens_run_loglik_ref)."""
        return self._loglik("run_loglik", obs_var, obs_tidx, obs_value, obs_sigma, normalize, on_device, reference)

    def summary(self, var, tidx: int) -> Dict[str, float]:
        out = np.empty(4)
        L.check(self._lib.rscm_ens_summary(self._h, self._var(var), tidx, L.dptr(out)))
        cnt = out[0]
        return {"count": int(cnt), "mean": out[1] / cnt if cnt else float("nan"),
                "min": out[2], "max": out[3]}

    def summary_series(self, var, t_begin: int = 0, t_end: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Ensemble count / mean / min / max over the finite members at every time index of
        ``[t_begin, t_end)`` -- the plume of a variable -- reduced on the device in two launches."""
        t_end = self.n_times if t_end is None else t_end
        out = np.empty((max(0, t_end - t_begin), 4))
        L.check(self._lib.rscm_ens_summary_series(self._h, self._var(var), t_begin, t_end, L.dptr(out)))
        cnt = out[:, 0]
        with np.errstate(all="ignore"):
            mean = np.where(cnt > 0, out[:, 1] / np.where(cnt > 0, cnt, 1.0), np.nan)
        return {"count": cnt.astype(np.int64), "mean": mean, "min": out[:, 2].copy(), "max": out[:, 3].copy()}

    def quantile_series(self, var, q, t_begin: int = 0, t_end: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Ensemble quantiles at every time index of ``[t_begin, t_end)``, reduced on the device:
        ``numpy.nanquantile(series[t], q)`` (linear method) per row.  Returns ``{"count": [rows],
        "quantiles": [rows][len(q)]}``."""
        qq = np.atleast_1d(L.f64(q))
        t_end = self.n_times if t_end is None else t_end
        rows = max(0, t_end - t_begin)
        out, cnt = np.empty((rows, qq.size)), np.empty(rows)
        L.check(self._lib.rscm_ens_quantile_series(self._h, self._var(var), t_begin, t_end, qq.size, L.dptr(qq), L.dptr(out), L.dptr(cnt)))
        return {"count": cnt.astype(np.int64), "quantiles": out}

    def quantile_rows(self, var, q, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                      weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``quantile_series``'s numbers over the rows ``t_begin, t_begin + t_stride, ... < t_end`` of any storage layout: full
        series, the window of a windowed handle or its output store (rscm_ens_quantile_rows_ex: the radix select that
        ``quantile_series`` runs on full storage, so the same bits, signed zeros included; up to 128 quantiles a call).
        Returns ``{"count": [rows], "quantiles": [rows][len(q)]}``.

        ``weighted``: ``numpy.nanquantile(row, q, weights=w, method="inverted_cdf")`` with the member weights
        (``set_member_weights`` / ``set_weights_from_loglik``; RSCM_SELECT_WEIGHTED).  Returns
        ``{"weight": [rows] (summed weight of the non-NaN members), "quantiles": [rows][len(q)]}``.

        ``anomaly``: the same quantiles of each member's own anomaly ``x[i] - b[i]`` against the baseline (``set_baseline``;
        RSCM_SELECT_ANOMALY) -- not the plume minus a quantile of the baseline.

        ``grouped``: one result per member group (``set_member_groups``; RSCM_SELECT_GROUPED), each exactly what the call
        returns for an ensemble of that group's members alone, from one series of passes over the rows.  Group-major:
        ``{"count" | "weight": [G][rows], "quantiles": [G][rows][len(q)]}``."""
        qq = np.atleast_1d(L.f64(q))
        t_end = self.n_times if t_end is None else t_end
        rows = len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0
        G = self._n_groups(grouped)
        out, cnt = np.empty((rows, G, qq.size)), np.empty((rows, G))
        flags = select_flags(weighted, anomaly, grouped)
        L.check(self._lib.rscm_ens_quantile_rows_ex(self._h, self._var(var), t_begin, t_end, t_stride, qq.size, L.dptr(qq), flags,
                                                    L.dptr(out), L.dptr(cnt)))
        return select_result(out, cnt, weighted, grouped)

    def select(self, var, q, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
               weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> "QuantileSelect":
        """``quantile_rows`` in stages, for a caller that sums the histograms of several handles between the passes (the
        shards of one ensemble: ``rscm_amd.distributed.quantile_rows_global``).  Use as a context manager.  ``weighted``: the
        weighted select; ``result()`` then returns ``{"weight", "quantiles"}``.  ``anomaly``: of the anomalies against the
        baseline.  ``grouped``: per member group; every handle of one sharded select must carry the same number of groups."""
        return QuantileSelect(self, var, q, t_begin, t_end, t_stride, weighted, anomaly, grouped=grouped)

    # -- baseline, per-member indicators, exceedance ------------------------------------------
    def set_baseline(self, var, t_begin: int, t_end: int, t_stride: int = 1) -> None:
        """The baseline ``b[i]``: member i's mean of ``var`` over the rows ``t_begin, t_begin + t_stride, ... < t_end`` (the sum
        in row order divided by the row count; NaN if any of its rows is), computed on the device and kept by the handle
        across ``run`` and ``rewind``.  ``quantile_rows(..., anomaly=True)`` and ``indicators(..., anomaly=True)`` read it."""
        L.check(self._lib.rscm_ens_set_baseline(self._h, self._var(var), int(t_begin), int(t_end), int(t_stride)))

    def set_baseline_values(self, b) -> None:
        """The baseline from ``[N]`` float64 values: a numpy array or a ``DeviceVector`` on this ensemble's GPU."""
        if isinstance(b, DeviceVector):
            if b.n != self.n_members or b.dtype != np.float64:
                raise ValueError(f"baseline: need a float64 device vector of {self.n_members} members")
            L.check(self._lib.rscm_ens_set_baseline_values(self._h, C.cast(C.c_void_p(b.ptr), C.POINTER(C.c_double)), 1))
            return
        a = np.ascontiguousarray(b, dtype=np.float64)
        if a.shape != (self.n_members,):
            raise ValueError(f"baseline: need {self.n_members} values, got shape {a.shape}")
        L.check(self._lib.rscm_ens_set_baseline_values(self._h, L.dptr(a), 0))

    def baseline_device(self) -> DeviceVector:
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_baseline_devptr(self._h, C.byref(p)))
        return DeviceVector(p.value, self.n_members, np.float64, self)

    def baseline(self) -> np.ndarray:
        """The baseline, ``[N]`` float64, copied to the host."""
        return self.baseline_device().to_host()

    def clear_baseline(self) -> None:
        L.check(self._lib.rscm_ens_clear_baseline(self._h))

    def _slot_vectors(self, p, count: int) -> List[DeviceVector]:
        """The first ``count`` rows of the indicator slot at ``p`` (a ``c_void_p`` an entry point filled) as ``DeviceVector``s of ``[N]`` float64."""
        n = self.n_members
        return [DeviceVector(p.value + 8 * n * j, n, np.float64, self) for j in range(count)]

    @staticmethod
    def _band_edge_array(bands, n: int, max_bands: Optional[int] = None) -> np.ndarray:
        """``bands`` -- a count (at most ``max_bands`` where given; ``band_edges`` then gives the edges for ``n`` terms) or explicit
        edges -- as the contiguous int32 edge array the C boundary takes."""
        from .variability import band_edges
        if isinstance(bands, (int, np.integer)):
            if max_bands is not None and not 1 <= int(bands) <= max_bands:
                raise ValueError(f"bands: 1 to {max_bands} bands per call, got {int(bands)}")
            return band_edges(n, int(bands)) if n >= 3 else np.array([1, 2], dtype=np.int32)    # (too short a series: the call refuses it)
        edges = np.ascontiguousarray(np.asarray(bands, dtype=np.int32).ravel())
        if edges.size < 2:
            raise ValueError("bands: an explicit edge list needs at least two edges")
        return edges

    def indicators(self, var, t_begin: int, t_end: int, t_stride: int = 1, thresholds=(), anomaly: bool = False,
                   slot: int = 0) -> Dict[str, object]:
        """Per-member indicators of ``var`` over the rows ``t_begin, t_begin + t_stride, ... < t_end`` (of the anomaly against
        the baseline with ``anomaly``), left on the device in indicator slot ``slot`` (0-3; each slot's vectors stay valid
        until its next use): ``{"mean", "peak", "peak_time", "crossing": [one per threshold]}``, ``DeviceVector``s of ``[N]``
        float64.  ``peak_time`` is the time of the first row attaining the peak; ``crossing[k]`` that of the first row
        ``>= thresholds[k]`` (``inf`` if none).  A member with a NaN in any row has NaN in every indicator."""
        thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_indicators(self._h, self._var(var), int(t_begin), int(t_end), int(t_stride), int(bool(anomaly)),
                                                     thr.size, L.dptr(thr), int(slot), C.byref(p)))
        vec = self._slot_vectors(p, 3 + thr.size)
        return {"mean": vec[0], "peak": vec[1], "peak_time": vec[2], "crossing": vec[3:]}

    def variability(self, var, t_begin: int, t_end: int, t_stride: int = 1, detrend: str = "linear", slot: int = 0) -> Dict[str, object]:
        """Per-member variability statistics of ``var`` over the rows ``t_begin, t_begin + t_stride, ... < t_end``, left on the
        device in indicator slot ``slot`` (the slots of ``indicators``: a slot holds the vectors of the last call on it, of either
        kind): ``{"mean", "slope", "variance", "sd", "r1"}``, ``DeviceVector``s of ``[N]`` float64.  ``detrend``: ``"mean"`` --
        variance and lag-one autocorrelation ``r1`` about the member's mean; ``"linear"`` -- about its least-squares line, whose
        ``slope`` is per row (per ``t_stride`` steps); ``"difference"`` -- of the first differences of the rows (``mean`` is then
        the mean increment).  The definition is ``rscm_amd.variability.series_variability``'s, bit for bit (rscm_ens_member_variability).
        At least three terms; a member with a non-finite value in any row has NaN in all five."""
        from .variability import detrend_mode
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_variability(self._h, self._var(var), int(t_begin), int(t_end), int(t_stride), detrend_mode(detrend),
                                                      int(slot), C.byref(p)))
        return dict(zip(("mean", "slope", "variance", "sd", "r1"), self._slot_vectors(p, 5)))

    def covariability(self, x, y, t_begin: int, t_end: int, t_stride: int = 1, detrend_x: str = "linear", detrend_y: str = "linear",
                      lags: int = 0, slot: int = 0) -> Dict[str, object]:
        """Per-member covariability of the variables ``x`` and ``y`` (stored or diagnostic; they may be the same) over the rows
        ``t_begin, t_begin + t_stride, ... < t_end``, left on the device in indicator slot ``slot`` (the slots of ``indicators``,
        ``variability`` and ``spectrum``): ``{"var_x", "var_y", "cov", "corr", "slope", "lead": [r_+1 ..], "lag": [r_-1 ..]}``,
        ``DeviceVector``s of ``[N]`` float64, ``lead`` and ``lag`` lists of ``lags`` (0 to 3) vectors.  Each variable is detrended
        as ``variability`` detrends it (``detrend_x``, ``detrend_y``); when exactly one of the two is ``"difference"``, the other is
        taken at the midpoints ``(x[k] + x[k + 1]) / 2`` the differences span and then detrended by its own mode -- a year's heat
        uptake against that year's temperature.  ``corr`` is the correlation of the two residual series and ``slope`` the
        regression slope of ``y`` on ``x``; ``lead[l - 1]`` is their correlation with ``x`` leading ``y`` by ``l`` terms,
        ``lag[l - 1]`` with ``y`` leading.  The definition is ``rscm_amd.variability.series_covariability``'s, bit for bit
        (rscm_ens_member_covariability).  At least ``3 + lags`` terms; a member with a non-finite value in any row of either
        variable has NaN everywhere, a constant series NaN in ``corr`` and the lags."""
        from .variability import detrend_mode
        lags = int(lags)
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_covariability(self._h, self._var(x), self._var(y), int(t_begin), int(t_end), int(t_stride),
                                                        detrend_mode(detrend_x), detrend_mode(detrend_y), lags, int(slot), C.byref(p)))
        vec = self._slot_vectors(p, 5 + 2 * lags)
        return {"var_x": vec[0], "var_y": vec[1], "cov": vec[2], "corr": vec[3], "slope": vec[4], "lead": vec[5::2], "lag": vec[6::2]}

    def cross_spectrum(self, x, y, t_begin: int, t_end: int, t_stride: int = 1, detrend_x: str = "linear", detrend_y: str = "linear",
                       bands=3, slot: int = 0) -> Dict[str, object]:
        """Per-member co-spectra of the variables ``x`` and ``y`` (stored or diagnostic; they may be the same) in frequency bands over
        the rows ``t_begin, t_begin + t_stride, ... < t_end``, left on the device in indicator slot ``slot`` (the slots of
        ``indicators``, ``variability``, ``spectrum`` and ``covariability``): ``{"var_x", "var_y", "coherence2": [one per band],
        "gain": [..], "gain_quad": [..], "edges", "counts"}`` -- ``DeviceVector``s of ``[N]`` float64, and the band edges and the
        number of frequencies per band as int32 arrays.  The working series and residuals are ``covariability``'s (``detrend_x``,
        ``detrend_y``; next to a differenced partner a variable is taken at the midpoints), the frequencies and ``bands`` are
        ``spectrum``'s, with at most 3 bands per call: a count (``rscm_amd.variability.band_edges`` then gives the edges) or 2 to 4
        strictly ascending edges inside ``[1, J + 1]``; only the frequencies inside the edges are computed.  Per band,
        ``coherence2`` is the squared coherence of the two residual series, ``gain`` the in-phase transfer of ``y`` on ``x`` (the
        band's co-spectrum over the power of ``x``: uptake per degree) and ``gain_quad`` the out-of-phase part, positive where
        ``x`` leads ``y``.  The definition is ``rscm_amd.variability.series_cross_spectrum``'s, bit for bit
        (rscm_ens_member_cross_spectrum).  3 to 4096 terms; a member with a non-finite value in any row of either variable has NaN
        everywhere, a constant series NaN in the band vectors."""
        from .variability import detrend_mode
        mode_x, mode_y = detrend_mode(detrend_x), detrend_mode(detrend_y)
        n = len(range(int(t_begin), int(t_end), max(int(t_stride), 1))) - (1 if L.VAR_DIFFERENCE in (mode_x, mode_y) else 0)
        edges = self._band_edge_array(bands, n, L.XSPEC_MAX_BANDS)
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_cross_spectrum(self._h, self._var(x), self._var(y), int(t_begin), int(t_end), int(t_stride), mode_x,
                                                         mode_y, edges.size - 1, edges.ctypes.data_as(C.POINTER(C.c_int32)), int(slot),
                                                         C.byref(p)))
        vec = self._slot_vectors(p, 2 + 3 * (edges.size - 1))
        return {"var_x": vec[0], "var_y": vec[1], "coherence2": vec[2::3], "gain": vec[3::3], "gain_quad": vec[4::3], "edges": edges,
                "counts": np.diff(edges).astype(np.int32)}

    def loglik_vectors(self, vectors, values, sigmas, add_to: Optional[DeviceVector] = None) -> DeviceVector:
        """Gaussian log-likelihood per member over per-member device vectors (variability statistics, indicators,
        ``params_vector`` rows): ``sum_j -0.5 ((values[j] - vectors[j][i]) / sigmas[j])^2``, added onto ``add_to`` -- a device
        log-likelihood, typically ``loglik(..., on_device=True)``, which may be overwritten in place -- or onto zero.  No
        normalisation terms: they are the same for every member and cancel in the weights.  A non-finite statistic or ``add_to``
        gives ``-inf``.  The result is the handle's likelihood vector (rscm_ens_loglik_vectors_device)."""
        arr, n_vec = self._vectors(vectors)
        val, sig = np.atleast_1d(L.f64(values)), np.atleast_1d(L.f64(sigmas))
        if not (n_vec == len(val) == len(sig)):
            raise ValueError("vectors, values and sigmas differ in length")
        add = None
        if add_to is not None:
            add = self._vectors([add_to])[0][0]
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_loglik_vectors_device(self._h, n_vec, arr, L.dptr(val), L.dptr(sig), add, C.byref(p)))
        return DeviceVector(p.value, self.n_members, np.float64, self)

    def spectrum(self, var, t_begin: int, t_end: int, t_stride: int = 1, detrend: str = "difference", bands=8, slot: int = 0) -> Dict[str, object]:
        """Per-member power spectrum of ``var`` in frequency bands over the rows ``t_begin, t_begin + t_stride, ... < t_end``, left
        on the device in indicator slot ``slot`` (the slots of ``indicators`` and ``variability``): ``{"mean", "slope", "variance",
        "power": [one per band], "edges", "counts"}`` -- ``DeviceVector``s of ``[N]`` float64, and the band edges and the number of
        frequencies per band as int32 arrays.  ``detrend`` as ``variability`` (``mean``, ``slope`` and ``variance`` are its bits).
        ``bands``: how many bands (``rscm_amd.variability.band_edges`` then gives the edges; fewer come back when the series has
        fewer frequencies) or an explicit list of 2 to 9 strictly ascending edges inside ``[1, J + 1]``, ``J = (n - 1) // 2`` of
        the working series' ``n`` terms; band ``b`` holds the frequencies ``edges[b] <= j < edges[b + 1]`` (cycles per ``n``
        terms).  ``power[b]`` is the mean periodogram ordinate of the band, scaled so that white noise has its variance there.
        The definition is ``rscm_amd.variability.series_spectrum``'s, bit for bit (rscm_ens_member_spectrum).  3 to 4096 terms; a
        member with a non-finite value in any row has NaN everywhere."""
        from .variability import detrend_mode
        mode = detrend_mode(detrend)
        n = len(range(int(t_begin), int(t_end), max(int(t_stride), 1))) - (1 if mode == L.VAR_DIFFERENCE else 0)
        edges = self._band_edge_array(bands, n)
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_spectrum(self._h, self._var(var), int(t_begin), int(t_end), int(t_stride), mode, edges.size - 1,
                                                   edges.ctypes.data_as(C.POINTER(C.c_int32)), int(slot), C.byref(p)))
        vec = self._slot_vectors(p, 3 + edges.size - 1)
        return {"mean": vec[0], "slope": vec[1], "variance": vec[2], "power": vec[3:], "edges": edges,
                "counts": np.diff(edges).astype(np.int32)}

    def loglik_spectrum(self, power, record_power, counts, add_to: Optional[DeviceVector] = None) -> DeviceVector:
        """Spectral log-likelihood per member over band powers (``spectrum(...)["power"]``) given the record's band powers
        (``rscm_amd.variability.series_spectrum`` of the record with the same detrender and edges) and the bands' ``counts``:
        ``sum_b counts[b] (ln P_b - 2 ln(P_b + record_power[b]))`` -- member and record as two realisations of one spectrum, the
        F-ratio form of Whittle's likelihood, member-independent terms dropped -- added onto ``add_to`` (a device log-likelihood,
        which may be overwritten in place) or onto zero.  A band power that is non-finite or ``<= 0``, or a non-finite
        ``add_to``, gives ``-inf``.  The result is the handle's likelihood vector (rscm_ens_loglik_spectrum_device; to rounding,
        not to the bit: it takes logarithms)."""
        arr, n_vec = self._vectors(power)
        rec = np.atleast_1d(L.f64(record_power))
        cnt = np.ascontiguousarray(np.atleast_1d(np.asarray(counts, dtype=np.int32)))
        if not (n_vec == len(rec) == len(cnt)):
            raise ValueError("power, record_power and counts differ in length")
        add = None
        if add_to is not None:
            add = self._vectors([add_to])[0][0]
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_loglik_spectrum_device(self._h, n_vec, arr, L.dptr(rec), cnt.ctypes.data_as(C.POINTER(C.c_int32)), add,
                                                          C.byref(p)))
        return DeviceVector(p.value, self.n_members, np.float64, self)

    # -- diagnostic variables ------------------------------------------------------------------
    def define_diagnostic(self, name: str, terms) -> int:
        """A diagnostic variable ``name``: a per-member linear combination of this ensemble's stored variables that every method
        taking ``var`` then takes by name or id (``quantile_rows``, ``set_baseline``, ``indicators``, ``variability``,
        ``spectrum``, ``loglik``, ``summary``, ``get_series``) once ``compute_diagnostic`` has formed its rows.  ``terms``: a
        sequence of ``(var, param_row_or_None[, scale=1.0])``; member i's value in a row is ``w_0 x_0 + w_1 x_1 + ...`` summed left
        to right, ``x_k`` that row of ``var`` and ``w_k = scale * params[param_row][i]`` (``scale`` alone with ``None``), every
        product and sum rounded on its own (rscm_ens_define_diagnostic; at most 4 terms, 4 diagnostics).  Returns the new id."""
        if not isinstance(name, str) or not name:
            raise ValueError("a diagnostic needs a name")
        if name in self.var_ids:
            raise ValueError(f"variable name {name!r} is taken")
        tv, tr, ts = [], [], []
        for term in terms:
            term = tuple(term)
            if len(term) not in (2, 3):
                raise ValueError(f"term {term!r}: (var, param_row_or_None[, scale]) expected")
            if isinstance(term[0], str) and term[0] in self._diagnostic_names:
                raise ValueError(f"term {term!r}: a diagnostic combines stored variables, not diagnostics")
            tv.append(self._var(term[0]))
            tr.append(-1 if term[1] is None else int(term[1]))
            ts.append(float(term[2]) if len(term) == 3 else 1.0)
        tv, tr = (np.ascontiguousarray(x, dtype=np.int32) for x in (tv, tr))
        ts = L.f64(ts)
        vid = C.c_int32()
        L.check(self._lib.rscm_ens_define_diagnostic(self._h, len(tv), L.iptr(tv), L.iptr(tr), L.dptr(ts), C.byref(vid)))
        self.var_ids[name] = vid.value
        self._diagnostic_names[name] = vid.value
        return vid.value

    def define_heat_content(self, name: str = "Ocean Heat Content", scale: float = 1.0) -> int:
        """The ocean heat content of a two-layer ensemble (plain, mix or with noise rows alike) as a diagnostic:
        ``H = (scale * C) Ts + (scale * Cd) Td`` with the member's own heat capacities, parameter rows 4 and 5 -- in W yr m^-2
        at ``scale`` 1.  Over the Earth's surface (5.101e14 m^2, 3.156e7 s per year) 1 W yr m^-2 is 1.610e22 J: ``scale=16.10``
        gives ZJ.  The reference integrates this quantity and drops it; its first differences (``detrend="difference"``) are the
        year-to-year uptake."""
        if self.kind != L.KIND_TWO_LAYER:
            raise ValueError("define_heat_content: the two-layer kind only (its rows 4 and 5 are the heat capacities)")
        return self.define_diagnostic(name, [("Surface Temperature", 4, scale), ("Deep Ocean Temperature", 5, scale)])

    def define_energy_budget(self, quantity: str, name: Optional[str] = None, scale: float = 1.0) -> int:
        """A term of a two-layer member's energy budget as a diagnostic variable (plain, mix and every noise kind), read by name
        like any diagnostic once ``compute_diagnostic`` has formed its rows.  ``quantity``: ``"forcing"`` -- the forcing F the
        member saw, its scenario or mix sum with its noise; ``"response"`` -- ``(lambda0 - a Ts) Ts``; ``"deep_uptake"`` --
        ``eta (Ts - Td)``; ``"imbalance"`` -- the top-of-atmosphere imbalance ``N = F - response - (efficacy - 1) eta (Ts - Td)``,
        which is ``C dTs/dt + Cd dTd/dt``.  Row t holds the value at the start of the step out of row t, in W m^-2 times ``scale``
        (rscm_ens_define_energy_budget states the arithmetic).  ``name`` defaults to ``"Member Forcing"``, ``"Radiative
        Response"``, ``"Deep Ocean Heat Uptake"``, ``"Top of Atmosphere Imbalance"``.  ``"forcing"`` and ``"imbalance"`` go
        stale with ``set_forcing`` as well as with everything that makes a diagnostic stale, and are refused on an ensemble whose
        forcing is linked.  ``covariability("Surface Temperature", N)["slope"]`` is each member's Gregory slope.  Returns the id."""
        if quantity not in L.BUDGET_QUANTITIES:
            raise ValueError(f"unknown energy-budget quantity {quantity!r}; one of {sorted(L.BUDGET_QUANTITIES)}")
        name = L.BUDGET_DEFAULT_NAMES[quantity] if name is None else name
        if not isinstance(name, str) or not name:
            raise ValueError("a diagnostic needs a name")
        if name in self.var_ids:
            raise ValueError(f"variable name {name!r} is taken")
        vid = C.c_int32()
        L.check(self._lib.rscm_ens_define_energy_budget(self._h, L.BUDGET_QUANTITIES[quantity], float(scale), C.byref(vid)))
        self.var_ids[name] = vid.value
        self._diagnostic_names[name] = vid.value
        return vid.value

    def define_toa_imbalance(self, name: str = "Top of Atmosphere Imbalance", scale: float = 1.0) -> int:
        """``define_energy_budget("imbalance", name, scale)``: the quantity observations constrain the feedback through."""
        return self.define_energy_budget("imbalance", name, scale)

    def define_running_mean(self, name: str, source, window: int = 20, align: str = "centre", step: int = 1) -> int:
        """A diagnostic variable ``name``: the running mean of ``source`` -- a stored variable, or a linear or energy-budget
        diagnostic defined before (name or id) -- over ``window`` rows ``step`` time indices apart.  ``align``: ``"centre"`` (the
        window of row t starts ``(window - 1) // 2`` terms before it: 20 terms span t - 9 .. t + 10) or ``"trailing"`` (it ends at
        t).  The terms are added in time order, one float64 add each, and divided by ``float(window)``; there is no sliding update,
        so a non-finite source row reaches the rows whose window holds it and no other (rscm_ens_define_running_mean states the
        arithmetic; ``rscm_amd.variability.series_running_mean`` is the same estimator for a record).  Every method that takes
        ``var`` takes the name once ``compute_diagnostic`` has formed the rows: ``indicators`` gives the crossing of the 20-year
        mean, ``exceedance_rows`` its probability, ``loglik`` scores a decadal mean.  ``step=12`` averages every twelfth row of a
        monthly axis; ``step=1, window=12`` computed with ``t_stride=12`` gives annual means of monthly rows.  Window 2 .. 64;
        takes one of the 4 diagnostic slots.  Returns the new id."""
        if not isinstance(name, str) or not name:
            raise ValueError("a diagnostic needs a name")
        if name in self.var_ids:
            raise ValueError(f"variable name {name!r} is taken")
        if align not in L.RUNMEAN_ALIGN:
            raise ValueError(f"align must be one of {sorted(L.RUNMEAN_ALIGN)}, got {align!r}")
        vid = C.c_int32()
        L.check(self._lib.rscm_ens_define_running_mean(self._h, self._var(source), int(window), L.RUNMEAN_ALIGN[align], int(step), C.byref(vid)))
        self.var_ids[name] = vid.value
        self._diagnostic_names[name] = vid.value
        return vid.value

    def diagnostics_running_mean(self, vid: int) -> Optional[Dict[str, object]]:
        """The running-mean definition behind diagnostic ``vid`` as ``diagnostics`` reports it, ``None`` for another sort."""
        src, w, al, st = (C.c_int32() for _ in range(4))
        L.check(self._lib.rscm_ens_diagnostic_running_mean(self._h, vid, C.byref(src), C.byref(w), C.byref(al), C.byref(st)))
        if src.value == 0:
            return None
        return {"source": src.value, "window": w.value, "align": {v: k for k, v in L.RUNMEAN_ALIGN.items()}[al.value], "step": st.value}

    def running_mean_range(self, var, time_index: Optional[int] = None) -> Tuple[int, int]:
        """``(t_begin, t_end)`` of running-mean diagnostic ``var``: the first row whose window is complete, and one past the last
        row whose window ends at or below ``time_index`` (default: the ensemble's own).  What ``compute_diagnostic`` takes for
        ``None``.  ``t_end <= t_begin`` while no row has a full window."""
        rm = self.diagnostics_running_mean(self._var(var))
        if rm is None:
            raise ValueError(f"{var!r} is no running mean")
        from .variability import running_mean_back
        back = running_mean_back(rm["window"], rm["align"]) * rm["step"]
        ahead = (rm["window"] - 1) * rm["step"] - back
        return back, (self.time_index if time_index is None else int(time_index)) - ahead + 1

    def compute_diagnostic(self, var, t_begin: Optional[int] = None, t_end: Optional[int] = None, t_stride: int = 1) -> None:
        """Form the rows ``t_begin, t_begin + t_stride, ... < t_end`` of diagnostic ``var`` from the stored rows and the parameters
        as they stand (``t_begin=None``: row 0; ``t_end=None``: up to and including the current time index).  For a running mean
        (``define_running_mean``) ``t_begin=None`` is the first row with a full window and ``t_end=None`` one past the last row
        with a full window at or below the time index (``running_mean_range``); explicit values are passed through and may be
        refused -- no row is padded.  The rows are a snapshot: after anything that
        writes rows or parameters (``run``, ``rewind``, ``set_params``, ``restore``, being a ``branch`` destination, ...) readers
        are refused until the next ``compute_diagnostic`` (rscm_ens_compute_diagnostic).  One range at a time."""
        vid = self._var(var)
        if (t_begin is None or t_end is None) and vid >= self.n_vars and self.diagnostics_running_mean(vid) is not None:
            lo, hi = self.running_mean_range(vid)
            t_begin, t_end = (lo if t_begin is None else int(t_begin)), (hi if t_end is None else int(t_end))
        t_begin = 0 if t_begin is None else int(t_begin)
        t_end = self.time_index + 1 if t_end is None else int(t_end)
        L.check(self._lib.rscm_ens_compute_diagnostic(self._h, vid, t_begin, t_end, int(t_stride)))

    @property
    def diagnostics(self) -> Dict[str, Dict[str, object]]:
        """The definitions as the library holds them, by name: ``{"id", "terms": [(var id, param row or None, scale)],
        "rows_held", "t_begin", "t_stride", "quantity", "scale", "running_mean"}`` (``rows_held`` 0 when nothing is computed or the
        rows are stale; ``quantity`` is ``None`` and ``scale`` ``None`` for a linear diagnostic, the name of the energy-budget
        quantity and its scale for one of ``define_energy_budget``, whose ``terms`` are empty; ``running_mean`` is ``None``, or
        ``{"source": id, "window", "align", "step"}`` for one of ``define_running_mean``, whose ``terms`` are empty too)."""
        out = {}
        quantity_names = {v: k for k, v in L.BUDGET_QUANTITIES.items()}
        for name, vid in self._diagnostic_names.items():
            n, held, tb, st = (C.c_int32() for _ in range(4))
            tv, tr = np.zeros(L.DIAG_MAX_TERMS, dtype=np.int32), np.zeros(L.DIAG_MAX_TERMS, dtype=np.int32)
            ts = np.zeros(L.DIAG_MAX_TERMS)
            L.check(self._lib.rscm_ens_diagnostic(self._h, vid, C.byref(n), L.iptr(tv), L.iptr(tr), L.dptr(ts), C.byref(held), C.byref(tb),
                                                  C.byref(st)))
            out[name] = {"id": vid, "terms": [(int(tv[k]), None if tr[k] < 0 else int(tr[k]), float(ts[k])) for k in range(n.value)],
                         "rows_held": held.value, "t_begin": tb.value, "t_stride": st.value}
            q, qs = C.c_int32(), C.c_double()
            L.check(self._lib.rscm_ens_diagnostic_quantity(self._h, vid, C.byref(q), C.byref(qs)))
            out[name]["quantity"] = quantity_names.get(q.value)
            out[name]["scale"] = qs.value if q.value else None
            out[name]["running_mean"] = self.diagnostics_running_mean(vid)
        return out

    def clear_diagnostics(self) -> None:
        """Remove every diagnostic: definitions, rows and names."""
        L.check(self._lib.rscm_ens_clear_diagnostics(self._h))
        for name in self._diagnostic_names:
            del self.var_ids[name]
        self._diagnostic_names = {}

    def _vectors(self, vectors):
        vs = list(vectors)
        for v in vs:
            if not isinstance(v, DeviceVector) or v.n != self.n_members or v.dtype != np.float64:
                raise ValueError(f"vectors: need float64 DeviceVectors of {self.n_members} members")
        arr = (C.POINTER(C.c_double) * len(vs))(*[C.cast(C.c_void_p(v.ptr), C.POINTER(C.c_double)) for v in vs])
        return arr, len(vs)

    def quantile_vectors(self, vectors, q, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``quantile_rows``' quantiles with device vectors of ``[N]`` float64 as the rows: indicators, parameter rows
        (``params_vector``), a log-likelihood.  Returns ``{"count" | "weight": [len(vectors)], "quantiles": [len(vectors)][len(q)]}``;
        with ``grouped`` per member group, group-major as ``quantile_rows``."""
        arr, n_vec = self._vectors(vectors)
        qq = np.atleast_1d(L.f64(q))
        G = self._n_groups(grouped)
        out, cnt = np.empty((n_vec, G, qq.size)), np.empty((n_vec, G))
        L.check(self._lib.rscm_ens_quantile_vectors(self._h, n_vec, arr, qq.size, L.dptr(qq), select_flags(weighted, False, grouped),
                                                    L.dptr(out), L.dptr(cnt)))
        return select_result(out, cnt, weighted, grouped)

    def select_vectors(self, vectors, q, weighted: bool = False, grouped: bool = False) -> "QuantileSelect":
        """``quantile_vectors`` in stages (``select``'s protocol): ``rscm_amd.distributed.quantile_vectors_global``."""
        return QuantileSelect(self, None, q, 0, None, 1, weighted, vectors=vectors, grouped=grouped)

    # -- member groups (the grouped quantiles and exceedance) ----------------------------------
    def set_member_groups(self, groups, n_groups: Optional[int] = None) -> None:
        """Member groups for the ``grouped=True`` statistics: ``[N]`` int32 ids, -1 (the member is in no group) or
        ``0 <= id < n_groups <= 64``; a numpy array or an int32 ``DeviceVector`` on this ensemble's GPU.  ``n_groups`` defaults to
        ``max + 1`` for host arrays.  They stay across ``run``, ``rewind`` and a ``branch`` into this ensemble."""
        if isinstance(groups, DeviceVector):
            if groups.n != self.n_members or groups.dtype != np.int32:
                raise ValueError(f"groups: need an int32 device vector of {self.n_members} members")
            if n_groups is None:
                raise ValueError("groups: n_groups is needed with a device vector")
            L.check(self._lib.rscm_ens_set_member_groups(self._h, C.cast(C.c_void_p(groups.ptr), C.POINTER(C.c_int32)), 1, int(n_groups)))
            return
        a = np.asarray(groups)
        if a.shape != (self.n_members,):
            raise ValueError(f"groups: need {self.n_members} values, got shape {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("groups must be integers")
        if n_groups is None:
            n_groups = max(int(a.max()) + 1, 1)
        a = np.ascontiguousarray(a, dtype=np.int32)
        L.check(self._lib.rscm_ens_set_member_groups(self._h, L.iptr(a), 0, int(n_groups)))

    def member_groups_device(self) -> DeviceVector:
        """The group ids as an int32 ``DeviceVector`` carrying ``n_groups``."""
        p, g = C.c_void_p(), C.c_int32(0)
        L.check(self._lib.rscm_ens_member_groups_devptr(self._h, C.byref(p), C.byref(g)))
        v = DeviceVector(p.value, self.n_members, np.int32, self)
        v.n_groups = g.value
        return v

    def member_groups(self) -> np.ndarray:
        """The member groups, ``[N]`` int32, copied to the host."""
        return self.member_groups_device().to_host()

    @property
    def n_groups(self) -> int:
        """The number of member groups set, 0 if none."""
        p, g = C.c_void_p(), C.c_int32(0)
        self._lib.rscm_ens_member_groups_devptr(self._h, C.byref(p), C.byref(g))
        return g.value

    def clear_member_groups(self) -> None:
        L.check(self._lib.rscm_ens_clear_member_groups(self._h))

    def _n_groups(self, grouped: bool) -> int:
        """The group dimension of a result buffer: 1 without ``grouped`` (and without groups: the library then refuses the call)."""
        return max(self.n_groups, 1) if grouped else 1

    def exceedance(self, vector, thresholds, weighted: bool = False, grouped: bool = False) -> Dict[str, object]:
        """Exceedance of a ``[N]`` float64 ``DeviceVector``: ``{"hits": [k] int64 (members, or with ``weighted`` their summed
        weight, with ``v >= thresholds[k]``), "total": int64 (non-NaN members or their weight), "probability": hits / total}``
        (NaN where total is 0).  Integer sums, so those of shards add up to the whole ensemble's.  ``grouped``: per member group,
        ``{"hits": [G][k], "total": [G], "probability": [G][k]}``."""
        (arr, _n) = self._vectors([vector])
        thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        if grouped:
            G = self._n_groups(True)
            ghits, gtotal = np.zeros((G, thr.size), dtype=np.int64), np.zeros(G, dtype=np.int64)
            L.check(self._lib.rscm_ens_exceedance_grouped(self._h, arr[0], thr.size, L.dptr(thr), int(bool(weighted)),
                                                          ghits.ctypes.data_as(C.POINTER(C.c_int64)),
                                                          gtotal.ctypes.data_as(C.POINTER(C.c_int64))))
            return exceedance_grouped_result(ghits, gtotal)
        hits, total = np.zeros(thr.size, dtype=np.int64), C.c_int64(0)
        L.check(self._lib.rscm_ens_exceedance(self._h, arr[0], thr.size, L.dptr(thr), int(bool(weighted)),
                                              hits.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total)))
        return exceedance_result(hits, total.value)

    def moment_sums(self, vectors, order: int, center=None, weighted: bool = False, grouped: bool = False) -> np.ndarray:
        """The exact integer sums behind ``moments`` (rscm_ens_moment_sums) of up to eight ``[N]`` float64 ``DeviceVector``s:
        int64 ``[G][2 + B * 69]``, per group the count n, the weight W and B blocks of 68 limbs and a count of non-finite terms --
        ``order`` 1: B = K, the sums of w x; 2: B = K (K + 1) / 2, the sums of w (x_a - c_a)(x_b - c_b) about ``center`` ``[G][K]``
        for a <= b.  G is 1 without ``grouped``.  The arrays of shards add up element by element; ``moments_result`` finishes them."""
        arr, n_vec = self._vectors(vectors)
        if not 1 <= n_vec <= L.MOMENT_MAX_VECTORS:
            raise ValueError(f"moments: 1 to {L.MOMENT_MAX_VECTORS} vectors, got {n_vec}")
        c, out = _moment_sums_args("moments", order, center, (self._n_groups(grouped), n_vec), moment_blocks(n_vec, order))
        L.check(self._lib.rscm_ens_moment_sums(self._h, n_vec, arr, select_flags(weighted, False, grouped), int(order),
                                               None if c is None else L.dptr(c), out.ctypes.data_as(C.POINTER(C.c_int64)), 0))
        return out

    def moments(self, vectors, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Exact weighted mean vector and covariance matrix of up to eight ``[N]`` float64 ``DeviceVector``s over the members
        (indicators, ``params_vector`` rows, a log-likelihood): ``{"count", "weight", "mean": [K], "cov": [K][K], "sd": [K],
        "corr": [K][K]}``, with ``grouped`` per member group, the group dimension leading.  A member counts when all K of its
        values are finite; ``weighted`` takes the member weights as frequencies (the divisor is their sum W).  Every mean and
        covariance is the exact sum, accumulated in integers on the device, divided by W and rounded once, so the result has
        the same bits whatever the order of the members, and ``rscm_amd.distributed.moments_global`` returns them for a sharded
        ensemble.  W == 0: NaN."""
        arr, K = self._vectors(vectors)
        if not 1 <= K <= L.MOMENT_MAX_VECTORS:
            raise ValueError(f"moments: 1 to {L.MOMENT_MAX_VECTORS} vectors, got {K}")
        G = self._n_groups(grouped)
        mean, cov = np.empty((G, K)), np.empty((G, K, K))
        n, w = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_moments(self._h, K, arr, select_flags(weighted, False, grouped), L.dptr(mean), L.dptr(cov),
                                           n.ctypes.data_as(i64), w.ctypes.data_as(i64)))
        return moments_dict(n, w, mean, cov, grouped)

    def _moment_rows_args(self, var, t_begin, t_end, t_stride, vectors):
        arr, K = self._vectors(vectors)
        if K > L.MOMENT_ROWS_MAX_VECTORS:
            raise ValueError(f"moment_rows: at most {L.MOMENT_ROWS_MAX_VECTORS} vectors, got {K}")
        t_end = self.n_times if t_end is None else t_end
        rows = len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0
        return self._var(var), t_end, rows, (arr if K else None), K

    def moment_rows_sums(self, var, order: int, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, vectors=(), center=None,
                         weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> np.ndarray:
        """The exact integer sums behind ``moment_rows`` (rscm_ens_moment_rows_sums) over the rows ``t_begin, t_begin + t_stride, ...
        < t_end`` of ``var`` and up to four ``[N]`` float64 ``DeviceVector``s: int64 ``[rows][G][2 + B * 69]``, per row and group the
        count n, the weight W and B blocks of 68 limbs and a count of non-finite terms -- ``order`` 1: B = 1 + K, the sums of w x and
        w v_k; 2: B = 1 + 2 K, the sums of the products xx, x v_k, v_k v_k of the differences from ``center`` ``[rows][G][1 + K]``.
        G is 1 without ``grouped``.  The arrays of shards add up element by element; ``moment_rows_result`` finishes them."""
        vid, t_end, rows, arr, K = self._moment_rows_args(var, t_begin, t_end, t_stride, vectors)
        c, out = _moment_sums_args("moment_rows", order, center, (rows, self._n_groups(grouped), 1 + K), moment_rows_blocks(K, order))
        L.check(self._lib.rscm_ens_moment_rows_sums(self._h, vid, t_begin, t_end, t_stride, K, arr, select_flags(weighted, anomaly, grouped),
                                                    int(order), None if c is None else L.dptr(c), out.ctypes.data_as(C.POINTER(C.c_int64)), 0))
        return out

    def moment_rows(self, var, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, vectors=(), weighted: bool = False,
                    anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """The plume as mean and spread: the exact weighted mean and variance of ``var`` across members at every row ``t_begin,
        t_begin + t_stride, ... < t_end``, read wherever the rows are resident (full series, window, output store), and its
        covariance with up to four ``[N]`` float64 ``DeviceVector``s (a parameter row, an indicator).  Returns ``{"count", "weight",
        "mean", "var", "sd": [rows]}`` and, with vectors, ``{"vec_mean", "vec_var", "cov", "corr", "slope": [rows][K]}``: ``slope =
        cov / vec_var`` is the row regressed on the vector, that year's value per unit of the parameter.  A member counts in a row
        when its value there and all its vector values are finite, so every row has its own count; ``weighted`` takes the member
        weights as frequencies, ``anomaly`` the member's value minus its baseline (the bits ``quantile_rows(anomaly=True)`` sees),
        ``grouped`` gives one result per member group, the group dimension after rows.  Every mean, variance and covariance is the
        exact sum, accumulated in integers on the device, over W, rounded once: the same bits for any order of the members, and
        ``rscm_amd.distributed.moment_rows_global`` returns them for a sharded ensemble.  Rows beyond the time index: count 0, NaN."""
        vid, t_end, rows, arr, K = self._moment_rows_args(var, t_begin, t_end, t_stride, vectors)
        G = self._n_groups(grouped)
        mean, second = np.empty((rows, G, 1 + K)), np.empty((rows, G, 1 + 2 * K))
        n, w = np.zeros((rows, G), dtype=np.int64), np.zeros((rows, G), dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_moment_rows(self._h, vid, t_begin, t_end, t_stride, K, arr, select_flags(weighted, anomaly, grouped),
                                               L.dptr(mean), L.dptr(second), n.ctypes.data_as(i64), w.ctypes.data_as(i64)))
        return moment_rows_dict(n, w, mean, second, grouped)

    def _exceedance_rows_sums(self, var, thr, per_row, t_begin, t_end, t_stride, weighted, anomaly, grouped, with_equal):
        """rscm_ens_exceedance_rows: int64 ``hits[rows][G][K]``, ``equal`` (None unless asked for) and ``total[rows][G]``."""
        G = self._n_groups(grouped)
        rows = len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0
        K = thr.shape[-1]
        hits, total = np.zeros((rows, G, K), dtype=np.int64), np.zeros((rows, G), dtype=np.int64)
        equal = np.zeros((rows, G, K), dtype=np.int64) if with_equal else None
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_exceedance_rows(self._h, self._var(var), t_begin, t_end, t_stride, K, L.dptr(thr), int(per_row),
                                                   select_flags(weighted, anomaly, grouped), hits.ctypes.data_as(i64),
                                                   equal.ctypes.data_as(i64) if with_equal else None, total.ctypes.data_as(i64)))
        return hits, equal, total

    def exceedance_rows(self, var, thresholds, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                        anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Exceedance as a series: at every row ``t_begin, t_begin + t_stride, ... < t_end`` of ``var``, read wherever the rows are
        resident, the members (with ``weighted`` their summed weight) at or above each threshold.  ``thresholds`` is ``[K]``, the
        same for every row, or ``[rows][K]``, 1 <= K <= 8; any other shape is a ``ValueError``.  Returns ``{"hits": [rows][K] int64,
        "total": [rows] int64 (the members that are not NaN in that row, or their weight), "probability": hits / total}``, NaN where
        total is 0; with ``grouped`` per member group, the group axis after the rows.  ``anomaly`` takes the member's value minus its
        baseline (the bits ``quantile_rows(anomaly=True)`` sees).  A NaN threshold gives hits 0 and leaves total alone.  Integer
        sums in one launch for all rows: exact, so those of shards add up (``rscm_amd.distributed.exceedance_rows_global``).  Rows
        beyond the time index: zeros, NaN."""
        t_end = self.n_times if t_end is None else t_end
        thr, per_row = exceedance_rows_thresholds(thresholds, len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0)
        hits, _, total = self._exceedance_rows_sums(var, thr, per_row, t_begin, t_end, t_stride, weighted, anomaly, grouped, False)
        return exceedance_rows_result(hits, total, grouped)

    def rank_rows(self, var, record, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                  anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Where a record lies inside the plume: for every row the summed weight of the members below the observed value
        (``below``), equal to it (``equal``) and of all members that are not NaN there (``total``), int64 ``[rows]``, and the
        mid-rank ``pit = (2 below + equal) / (2 total)``, the record's probability integral transform.  ``record`` is ``[rows]``;
        NaN marks a row without an observation (``below = total``, ``equal = 0``, ``pit`` NaN).  ``rank_histogram`` bins the rows.
        Flags, rows and exactness as ``exceedance_rows``, whose kernel this is with the record as the per-row threshold."""
        t_end = self.n_times if t_end is None else t_end
        rec = rank_rows_record(record, len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0)
        hits, equal, total = self._exceedance_rows_sums(var, rec[:, None], True, t_begin, t_end, t_stride, weighted, anomaly, grouped, True)
        return rank_rows_result(hits[..., 0], equal[..., 0], total, rec, grouped)

    def histogram_rows(self, var, edges, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                       anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """The plume as a density over value and time: at every row ``t_begin, t_begin + t_stride, ... < t_end`` of ``var``, read
        wherever the rows are resident, the members (with ``weighted`` their summed weight) in each of the ``B = E - 1`` bins
        between ``edges`` (``[E]``, finite and strictly ascending, 2 <= E <= 1025): ``numpy.histogram``'s bins, the last edge
        closed.  Returns ``{"counts": [rows][B], "below", "above", "total": [rows] int64, "probability": counts / total}``, NaN
        where total is 0; ``below`` and ``above`` hold what lies outside the edges, and ``total = below + sum(counts) + above`` the
        members that are not NaN in that row.  With ``grouped`` per member group, the group axis after the rows (at most 8192
        slots: groups x (B + 2)); ``anomaly`` takes the member's value minus its baseline.  Integer sums in one launch for all
        rows: exact, so those of shards add up (``rscm_amd.distributed.histogram_rows_global``).  Bad edges are a ``ValueError``
        before any library call.  Rows beyond the time index: zeros, NaN."""
        t_end = self.n_times if t_end is None else t_end
        e = histogram_edges(edges, "histogram_rows: edges")
        G, rows, B = self._n_groups(grouped), (len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0), e.size - 1
        counts = np.zeros((rows, G, B), dtype=np.int64)
        below, above, total = (np.zeros((rows, G), dtype=np.int64) for _ in range(3))
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_histogram_rows(self._h, self._var(var), t_begin, t_end, t_stride, e.size, L.dptr(e),
                                                  select_flags(weighted, anomaly, grouped), counts.ctypes.data_as(i64),
                                                  below.ctypes.data_as(i64), above.ctypes.data_as(i64), total.ctypes.data_as(i64)))
        return histogram_result(counts, below, above, total, grouped)

    def histogram_vectors(self, vectors, edges, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``histogram_rows`` with 1 to 8 ``[N]`` float64 ``DeviceVector``s as the rows: the posterior density of a parameter
        (``params_vector``) or of an indicator.  ``edges`` is ``[E]``, shared, or ``[len(vectors)][E]``, one table per vector
        (parameters have different ranges); any other shape is a ``ValueError``.  NaN is left out per vector.  Returns the dict
        of ``histogram_rows`` with the vectors as the leading axis."""
        arr, n_vec = self._vectors(vectors)
        if not 1 <= n_vec <= L.HISTOGRAM_MAX_VECTORS:
            raise ValueError(f"histogram_vectors: 1 to {L.HISTOGRAM_MAX_VECTORS} vectors, got {n_vec}")
        e = histogram_edges(edges, "histogram_vectors: edges", n_vec)
        G, B = self._n_groups(grouped), e.shape[-1] - 1
        counts = np.zeros((n_vec, G, B), dtype=np.int64)
        below, above, total = (np.zeros((n_vec, G), dtype=np.int64) for _ in range(3))
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_histogram_vectors(self._h, n_vec, arr, e.shape[-1], L.dptr(e), int(e.ndim == 2),
                                                     select_flags(weighted, False, grouped), counts.ctypes.data_as(i64),
                                                     below.ctypes.data_as(i64), above.ctypes.data_as(i64), total.ctypes.data_as(i64)))
        return histogram_result(counts, below, above, total, grouped)

    def histogram2d(self, x, y, edges_x, edges_y, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """The joint density of two ``[N]`` float64 ``DeviceVector``s, one panel of a corner plot: ``{"counts": [Bx][By] int64,
        "outside", "total": int64, "probability": counts / total}``.  A member takes part when neither value is NaN; it counts in
        ``counts`` when both values fall into a bin of their edges (``numpy.histogram2d``'s bins) and in ``outside`` otherwise;
        ``total = sum(counts) + outside``.  With ``grouped`` per member group, the group axis leading (at most 8192 slots:
        groups x (Bx By + 1))."""
        arr, _n = self._vectors([x, y])
        ex, ey = histogram_edges(edges_x, "histogram2d: edges_x"), histogram_edges(edges_y, "histogram2d: edges_y")
        G = self._n_groups(grouped)
        counts = np.zeros((G, ex.size - 1, ey.size - 1), dtype=np.int64)
        outside, total = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        L.check(self._lib.rscm_ens_histogram2d(self._h, arr[0], arr[1], ex.size, L.dptr(ex), ey.size, L.dptr(ey),
                                               select_flags(weighted, False, grouped), counts.ctypes.data_as(i64),
                                               outside.ctypes.data_as(i64), total.ctypes.data_as(i64)))
        return histogram2d_result(counts, outside, total, grouped)

    def params_vector(self, row: int) -> DeviceVector:
        """Parameter row ``row`` of the ``[P][N]`` block as a ``DeviceVector`` (rscm_ens_params_devptr), e.g. for
        ``quantile_vectors``.  Once handed out, the block is read per member for the handle's life."""
        if not (0 <= row < self.n_params):
            raise ValueError(f"parameter row {row} out of range")
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_params_devptr(self._h, C.byref(p)))
        return DeviceVector(p.value + 8 * self.n_members * row, self.n_members, np.float64, self)

    # -- member weights (the weighted quantiles) ---------------------------------------------
    def set_member_weights(self, w) -> None:
        """Integer member weights for ``quantile_rows(..., weighted=True)``: ``[N]`` int64 >= 0, a numpy array or an int64
        ``DeviceVector`` (device memory on this ensemble's GPU).  They stay across ``run`` and ``rewind``."""
        if isinstance(w, DeviceVector):
            if w.n != self.n_members or w.dtype != np.int64:
                raise ValueError(f"weights: need an int64 device vector of {self.n_members} members")
            L.check(self._lib.rscm_ens_set_member_weights(self._h, C.cast(C.c_void_p(w.ptr), C.POINTER(C.c_int64)), 1))
            return
        a = np.asarray(w)
        if a.shape != (self.n_members,):
            raise ValueError(f"weights: need {self.n_members} values, got shape {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("weights must be integers (quantise float weights first: set_weights_from_loglik)")
        a = np.ascontiguousarray(a, dtype=np.int64)
        L.check(self._lib.rscm_ens_set_member_weights(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), 0))

    def member_weights_device(self) -> DeviceVector:
        p = C.c_void_p()
        L.check(self._lib.rscm_ens_member_weights_devptr(self._h, C.byref(p)))
        return DeviceVector(p.value, self.n_members, np.int64, self)

    def member_weights(self) -> np.ndarray:
        """The member weights, ``[N]`` int64, copied to the host."""
        return self.member_weights_device().to_host()

    def _loglik_arg(self, ll):
        if isinstance(ll, DeviceVector):
            if ll.n != self.n_members or ll.dtype != np.float64:
                raise ValueError(f"log-likelihood: need a float64 device vector of {self.n_members} members")
            return C.cast(C.c_void_p(ll.ptr), C.POINTER(C.c_double)), 1, None
        a = np.ascontiguousarray(ll, dtype=np.float64)
        if a.shape != (self.n_members,):
            raise ValueError(f"log-likelihood: need {self.n_members} values, got shape {a.shape}")
        return L.dptr(a), 0, a

    def loglik_max(self, ll) -> float:
        """max ``ll`` over members with status ok and a finite value (``-inf`` if none); ``ll``: numpy or ``DeviceVector``."""
        p, on_dev, _keep = self._loglik_arg(ll)
        out = C.c_double()
        L.check(self._lib.rscm_ens_loglik_max(self._h, p, on_dev, C.byref(out)))
        return out.value

    def set_weights_from_loglik(self, ll, bits: Optional[int] = None, ll_max: Optional[float] = None,
                                n_total: Optional[int] = None):
        """Member weights ``llround(exp(min(ll - ll_max, 0)) * 2**bits)`` for ok members with a finite ``ll``, 0 otherwise.
        ``ll_max`` defaults to ``loglik_max(ll)``; ``bits`` to ``53 - ceil(log2(n_total))`` (52 for one member), which keeps
        every row's summed weight within 2^53; ``n_total`` (default: this ensemble's members) is the size of the whole ensemble
        when this one is a shard.  Returns the ``(ll_max, bits)`` used."""
        if ll_max is None:
            ll_max = self.loglik_max(ll)
        if bits is None:
            bits = default_weight_bits(self.n_members if n_total is None else n_total)
        p, on_dev, _keep = self._loglik_arg(ll)
        L.check(self._lib.rscm_ens_set_weights_from_loglik(self._h, p, on_dev, float(ll_max), int(bits)))
        return float(ll_max), int(bits)

    def weights_ess(self) -> float:
        """Effective sample size of the member weights, ``(sum w)^2 / sum w^2`` in float64 on the host (a diagnostic)."""
        w = self.member_weights().astype(np.float64)
        s2 = float(np.dot(w, w))
        return float(w.sum()) ** 2 / s2 if s2 > 0 else 0.0

    # -- posterior ensembles: weight statistics, systematic resampling, branching --------------
    def weights_stats(self) -> Dict[str, object]:
        """Exact statistics of the member weights, reduced on the device in integers: ``total`` (sum w), ``n_nonzero``,
        ``w_max`` and ``sum_sq`` (sum w^2, up to 2^106) as Python ints, and ``ess = total^2 / sum_sq`` formed once on the host
        from them (0.0 without weight).  The integers of shards add up to those of the whole ensemble
        (``distributed.weights_stats_global``)."""
        total, nnz, wmax = C.c_int64(), C.c_int64(), C.c_int64()
        sq = (C.c_uint64 * 2)()
        L.check(self._lib.rscm_ens_weights_stats(self._h, C.byref(total), C.byref(nnz), C.byref(wmax), sq))
        return weights_stats_result(total.value, nnz.value, wmax.value, (int(sq[0]) << 64) | int(sq[1]))

    def resample(self, n_draws: int, seed: int = 0, offset: Optional[int] = None, w_before: int = 0,
                 w_total: Optional[int] = None) -> DeviceVector:
        """Systematic resampling of the member weights in integer arithmetic (``rscm_ens_resample``): the ancestors (local
        member indices, int64, non-decreasing) of this ensemble's share of ``n_draws`` equally weighted draws, left on the
        device and valid until the next ``resample``.  ``offset`` (default: ``resample_offset(seed, w_total)``) is the integer
        start 0 <= s < W.  A shard of a larger ensemble passes the weight ``w_before`` of the members before its own and the
        global ``w_total``; the returned vector then holds the contiguous run of draws ``k_first .. k_first + len - 1``
        (attribute ``k_first``) whose ancestors this ensemble owns."""
        if w_total is None:
            w_total = self.weights_stats()["total"] + int(w_before)
        if offset is None:
            offset = resample_offset(seed, w_total)
        k_first, count, p = C.c_int64(), C.c_int64(), C.c_void_p()
        L.check(self._lib.rscm_ens_resample(self._h, int(n_draws), int(offset), int(w_before), int(w_total), C.byref(k_first),
                                            C.byref(count), C.byref(p)))
        v = DeviceVector(p.value or 0, count.value, np.int64, self)
        v.k_first = k_first.value
        return v

    def branch(self, dst: "Ensemble", ancestors, dst_offset: int = 0) -> None:
        """Members ``[dst_offset, dst_offset + len(ancestors))`` of ``dst`` become copies of this ensemble's members
        ``ancestors`` (an int64 ``DeviceVector`` of ``resample``, or integers on the host) at the current time index, on the
        device (``rscm_ens_gather_members``): parameters, the current rows, look-back rows, status and internal component
        state.  ``dst`` needs no ``set_params``; it keeps its own forcing, which is the point: give it the scenarios to
        project under.  Members of ``dst`` that no call has written are the caller's business."""
        if isinstance(ancestors, DeviceVector):
            if ancestors.dtype != np.int64:
                raise ValueError("ancestors: need an int64 device vector")
            n, ptr, on_dev, keep = ancestors.n, C.cast(C.c_void_p(ancestors.ptr), C.POINTER(C.c_int64)), 1, ancestors
        else:
            keep = np.ascontiguousarray(ancestors, dtype=np.int64)
            if keep.ndim != 1:
                raise ValueError("ancestors: need a vector of member indices")
            n, ptr, on_dev = keep.size, keep.ctypes.data_as(C.POINTER(C.c_int64)), 0
        L.check(self._lib.rscm_ens_gather_members(dst._h, int(dst_offset), self._h, ptr, on_dev, n))

    def posterior(self, factory, n_draws: int, seed: int = 0, scenarios: int = 1):
        """An equally weighted posterior ensemble ready to project: ``dst = factory(n_draws * scenarios)`` (an ``Ensemble`` of
        this kind on this axis, mode and device), the same ``n_draws`` resampled members gathered into each of the
        ``scenarios`` blocks.  Returns ``(dst, scenario_of_member)`` with ``scenario_of_member = repeat(arange(scenarios),
        n_draws)`` for the caller's ``dst.set_forcing(series, scenario_of_member)``.  The same vector becomes ``dst``'s member
        groups (``set_member_groups``), so ``dst.quantile_rows(var, q, grouped=True)`` is the plume per scenario.

        Copies of one ancestor stay identical for ever under a shared forcing.  Giving ``dst`` its own forcing noise
        (``dst.set_forcing_noise(sigma, seed)`` in ``factory`` or afterwards; the noise belongs to ``dst`` like the forcing and
        a branch leaves it alone) is what makes them diverge: member j of ``dst`` then draws the variability of its own index,
        whatever ancestor it copies.  The handle-wide ``sigma`` and ``phi`` do not travel, they are ``dst``'s numbers; a ``dst`` made
        with ``noise_params=True`` from a source that has the rows (``dst.set_forcing_noise_members(seed)``) inherits each
        ancestor's amplitude and persistence with its other parameter rows, and realises its own noise under its own seed."""
        n_draws, scenarios = int(n_draws), int(scenarios)
        if n_draws < 1 or scenarios < 1:
            raise ValueError("need n_draws >= 1 and scenarios >= 1")
        anc = self.resample(n_draws, seed)
        dst = factory(n_draws * scenarios)
        for sidx in range(scenarios):
            self.branch(dst, anc, sidx * n_draws)
        for name, d in self.diagnostics.items():   # the projection can be summarised the way the source is (rows: dst's to compute)
            if name in dst.var_ids:
                continue
            if d["running_mean"] is not None:   # after its source (ids are in order of definition); the source by name, dst's id
                rm = d["running_mean"]
                source = next(n for n, v in self.var_ids.items() if v == rm["source"])
                dst.define_running_mean(name, source, rm["window"], rm["align"], rm["step"])
            elif d["quantity"] is None:
                dst.define_diagnostic(name, d["terms"])
            else:
                dst.define_energy_budget(d["quantity"], name, d["scale"])
        scenario_of_member = np.repeat(np.arange(scenarios, dtype=np.int32), n_draws)
        if scenarios <= 64:   # more scenarios than the library has groups: the blocks stay ungrouped
            dst.set_member_groups(scenario_of_member, scenarios)
        return dst, scenario_of_member


def weights_stats_result(total: int, n_nonzero: int, w_max: int, sum_sq: int) -> Dict[str, object]:
    """The dict of ``Ensemble.weights_stats`` from exact integers; ``ess = total^2 / sum_sq`` as one correctly rounded division."""
    total, sum_sq = int(total), int(sum_sq)
    from fractions import Fraction
    ess = float(Fraction(total * total, sum_sq)) if sum_sq else 0.0
    return {"total": total, "n_nonzero": int(n_nonzero), "w_max": int(w_max), "sum_sq": sum_sq, "ess": ess}


def resample_offset(seed: int, w_total: int) -> int:
    """The integer offset ``floor(R * w_total / 2^64)`` of a seeded systematic draw, ``R`` one 64-bit word of the library's Philox
    stream (``rscm_gpu_resample_offset``; computed on the host, so every rank derives the same one)."""
    s = C.c_int64()
    L.check(L.load().rscm_gpu_resample_offset(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(w_total), C.byref(s)))
    return s.value


def exceedance_result(hits, total: int) -> Dict[str, object]:
    """``{"hits", "total", "probability"}`` from int64 sums; the probability is ``hits / total`` in float64, NaN when total is 0."""
    hits = np.asarray(hits, dtype=np.int64)
    total = int(total)
    prob = hits.astype(np.float64) / float(total) if total else np.full(hits.shape, np.nan)
    return {"hits": hits, "total": total, "probability": prob}


def exceedance_grouped_result(hits, total) -> Dict[str, object]:
    """The grouped form: ``hits[G][k]``, ``total[G]``; a group without weight has NaN probabilities."""
    hits, total = np.asarray(hits, dtype=np.int64), np.asarray(total, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = np.where(total[:, None] != 0, hits.astype(np.float64) / total.astype(np.float64)[:, None], np.nan)
    return {"hits": hits, "total": total, "probability": prob}


def exceedance_rows_thresholds(thresholds, rows: int):
    """The checked thresholds of ``Ensemble.exceedance_rows`` over ``rows`` rows: ``(float64 array, per_row)`` from ``[K]`` (the
    same for every row) or ``[rows][K]``, 1 <= K <= 8.  Any other shape is a ``ValueError``; no library call is made."""
    thr = np.asarray(thresholds, dtype=np.float64)
    K = thr.shape[-1] if thr.ndim in (1, 2) else 0
    if not 1 <= K <= L.EXCEEDANCE_ROWS_MAX_THRESHOLDS or (thr.ndim == 2 and thr.shape[0] != rows):
        raise ValueError(f"exceedance_rows: thresholds must be [K] or [{rows}][K] with 1 <= K <= {L.EXCEEDANCE_ROWS_MAX_THRESHOLDS}, "
                         f"got shape {thr.shape}")
    return np.ascontiguousarray(thr), thr.ndim == 2


def rank_rows_record(record, rows: int) -> np.ndarray:
    """The checked record of ``Ensemble.rank_rows`` over ``rows`` rows: float64 ``[rows]``, else a ``ValueError``."""
    rec = np.asarray(record, dtype=np.float64)
    if rec.shape != (rows,):
        raise ValueError(f"rank_rows: the record must be [{rows}], got shape {rec.shape}")
    return np.ascontiguousarray(rec)


def _int_ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """``num / den`` of non-negative int64 arrays of one shape as float64, each the exact quotient rounded once; NaN where den is 0."""
    out = np.full(num.shape, np.nan)
    ok = den != 0
    if max(int(num.max(initial=0)), int(den.max(initial=0))) <= 1 << 53:     # both convert exactly: one IEEE division
        out[ok] = num[ok].astype(np.float64) / den[ok].astype(np.float64)
    else:                                                                    # Python's int / int rounds the exact quotient once
        out[ok] = [n / d for n, d in zip(num[ok].tolist(), den[ok].tolist())]
    return out


def _rows_groups(a, lead: np.ndarray = None) -> np.ndarray:
    """int64 ``[rows][G]...``: an array whose group axis (of length 1) was dropped gets it back; ``lead`` is one that has it."""
    a = np.asarray(a, dtype=np.int64)
    if lead is not None:
        return a.reshape(lead.shape[:2])
    return a[:, None, :] if a.ndim == 2 else a


def exceedance_rows_result(hits, total, grouped: bool = True) -> Dict[str, np.ndarray]:
    """The dict of ``Ensemble.exceedance_rows`` from the (reduced) int64 sums ``hits[rows][G][K]`` and ``total[rows][G]`` (G = 1
    without groups; that axis may be absent): ``probability = hits / total``, the exact quotient rounded once, NaN where total is
    0.  Without ``grouped`` the group axis is dropped."""
    hits = _rows_groups(hits)
    total = _rows_groups(total, hits)
    out = {"hits": hits, "total": total, "probability": _int_ratio(hits, np.broadcast_to(total[..., None], hits.shape))}
    return out if grouped else {k: v[:, 0] for k, v in out.items()}


def rank_rows_result(hits, equal, total, record, grouped: bool = True) -> Dict[str, np.ndarray]:
    """The dict of ``Ensemble.rank_rows`` from the (reduced) int64 sums ``hits``, ``equal`` and ``total``, each ``[rows][G]`` (G = 1
    without groups; that axis may be absent), of ``Ensemble.exceedance_rows``' kernel with ``record[rows]`` as the per-row
    threshold: ``below = total - hits``, and the mid-rank ``pit = (2 below + equal) / (2 total)``, the exact quotient rounded
    once, NaN where the record is NaN or total is 0.  Without ``grouped`` the group axis is dropped."""
    total = np.asarray(total, dtype=np.int64)
    total = total[:, None] if total.ndim == 1 else total
    hits, equal = _rows_groups(hits, total), _rows_groups(equal, total)
    record = np.asarray(record, dtype=np.float64).reshape(total.shape[0])
    below = total - hits
    pit = _int_ratio(2 * below + equal, 2 * total)
    pit[np.isnan(record)] = np.nan
    out = {"below": below, "equal": equal, "total": total, "pit": pit}
    return out if grouped else {k: v[:, 0] for k, v in out.items()}


def rank_histogram(below, equal, total, n_bins: int, record=None) -> np.ndarray:
    """The rank histogram of ``Ensemble.rank_rows``' ``below``, ``equal`` and ``total`` (``[rows]``, or ``[rows][G]``): int64
    ``[n_bins]`` (``[G][n_bins]``), the number of rows whose mid-rank falls into each of ``n_bins`` equal bins of [0, 1], bin
    ``floor(n_bins (2 below + equal) / (2 total))`` in Python integers -- no float binning -- with the top edge (a record at or
    above every member) in the last bin.  A flat histogram says the plume is neither too narrow nor too wide.  Rows without
    weight (total 0) have no rank and are left out, and so are the rows whose ``record`` (``[rows]``, if given) is NaN: pass the
    record that ``rank_rows`` took, since a row without an observation reads ``below = total`` like one above every member."""
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError("rank_histogram: n_bins must be at least 1")
    below, equal, total = (np.asarray(a, dtype=np.int64) for a in (below, equal, total))
    if not (below.shape == equal.shape == total.shape and below.ndim in (1, 2)):
        raise ValueError("rank_histogram: below, equal and total must share one shape, [rows] or [rows][G]")
    has = np.ones(below.shape[0], dtype=bool) if record is None else ~np.isnan(np.asarray(record, dtype=np.float64).reshape(below.shape[0]))
    b2, e2, t2 = (a.reshape(a.shape[0], -1) for a in (below, equal, total))
    out = np.zeros((b2.shape[1], n_bins), dtype=np.int64)
    for r in np.flatnonzero(has):
        for g, (b, e, t) in enumerate(zip(b2[r].tolist(), e2[r].tolist(), t2[r].tolist())):
            if t > 0:
                out[g, min(n_bins * (2 * b + e) // (2 * t), n_bins - 1)] += 1
    return out if below.ndim == 2 else out[0]


def histogram_edges(edges, what: str = "edges", tables: Optional[int] = None) -> np.ndarray:
    """The checked edges of a histogram call as a contiguous float64 array: ``[E]``, or with ``tables`` also ``[tables][E]``; 2 <= E
    <= 1025, every table finite and strictly ascending.  Anything else is a ``ValueError``; no library call is made."""
    e = np.asarray(edges, dtype=np.float64)
    shapes = f"[E] or [{tables}][E]" if tables is not None else "[E]"
    if not (e.ndim == 1 or (tables is not None and e.ndim == 2 and e.shape[0] == tables)):
        raise ValueError(f"{what} must be {shapes}, got shape {e.shape}")
    if not 2 <= e.shape[-1] <= L.HISTOGRAM_MAX_EDGES:
        raise ValueError(f"{what}: 2 to {L.HISTOGRAM_MAX_EDGES} edges, got {e.shape[-1]}")
    if not (np.isfinite(e).all() and (e[..., 1:] > e[..., :-1]).all()):
        raise ValueError(f"{what} must be finite and strictly ascending")
    return np.ascontiguousarray(e)


def histogram_result(counts, below, above, total, grouped: bool = True) -> Dict[str, np.ndarray]:
    """The dict of ``Ensemble.histogram_rows`` and ``histogram_vectors`` from the (reduced) int64 sums ``counts[rows][G][B]`` and
    ``below``, ``above``, ``total`` ``[rows][G]`` (G = 1 without groups; that axis may be absent): ``probability = counts / total``,
    the exact quotient rounded once, NaN where total is 0.  Without ``grouped`` the group axis is dropped."""
    counts = _rows_groups(counts)
    below, above, total = (_rows_groups(a, counts) for a in (below, above, total))
    out = {"counts": counts, "below": below, "above": above, "total": total,
           "probability": _int_ratio(counts, np.broadcast_to(total[..., None], counts.shape))}
    return out if grouped else {k: v[:, 0] for k, v in out.items()}


def histogram2d_result(counts, outside, total, grouped: bool = True) -> Dict[str, np.ndarray]:
    """The dict of ``Ensemble.histogram2d`` from the (reduced) int64 sums ``counts[G][Bx][By]``, ``outside[G]`` and ``total[G]`` (G =
    1 without groups; that axis may be absent): ``probability = counts / total``, the exact quotient rounded once, NaN where total
    is 0.  Without ``grouped`` the group axis is dropped."""
    counts = np.asarray(counts, dtype=np.int64)
    counts = counts[None] if counts.ndim == 2 else counts
    outside, total = (np.asarray(a, dtype=np.int64).reshape(counts.shape[0]) for a in (outside, total))
    out = {"counts": counts, "outside": outside, "total": total,
           "probability": _int_ratio(counts, np.broadcast_to(total[:, None, None], counts.shape))}
    return out if grouped else {k: v[0] for k, v in out.items()}


def crps_bracket(hist, edges, record) -> Dict[str, np.ndarray]:
    """A rigorous bracket of the continuous ranked probability score of every row of a histogram against ``record``, without a sort:
    ``{"lower", "upper"}``, float64 of the shape of ``hist["total"]`` (``[rows]``, or ``[rows][G]``).  ``hist`` is the dict of
    ``histogram_rows`` or ``histogram_vectors`` (or ``histogram_result`` of reduced sums), ``edges`` its ``[E]`` edges (``[rows][E]``
    for per-vector edges), ``record`` is ``[rows]``.

    With ``C_k`` the weight below ``e[k]`` and ``T`` the total, the weighted empirical distribution ``F`` of the row satisfies
    ``C_k / T <= F(x) <= C_{k+1} / T`` inside bin k.  The record's bin is split at ``y``; left of ``y`` the CRPS integrates ``F^2``,
    right of it ``(1 - F)^2``.  ``lower`` is the sum of ``width (C_k / T)^2`` over the pieces left of ``y`` plus ``width (1 - C_{k+1}
    / T)^2`` over those right of it; ``upper`` swaps ``C_k`` and ``C_{k+1}``.  Everything is formed in ``fractions.Fraction``
    (differences of doubles are exact) and each bound is rounded once.  The bracket contains the CRPS of the weighted empirical
    distribution and is at most as wide as the widest bin; the exact score needs the sorted members.

    A row gives ``(nan, nan)`` when the bracket would not hold or means nothing: weight outside the edges (``below`` or ``above``
    non-zero), ``T == 0``, a NaN record, or a record outside ``[e[0], e[E-1]]``."""
    from fractions import Fraction
    counts = np.asarray(hist["counts"], dtype=np.int64)
    shape = counts.shape[:-1]
    rows, B = counts.shape[0], counts.shape[-1]
    c3 = counts.reshape(rows, -1, B)
    below, above, total = (np.asarray(hist[k], dtype=np.int64).reshape(rows, -1) for k in ("below", "above", "total"))
    e = np.asarray(edges, dtype=np.float64)
    rec = np.asarray(record, dtype=np.float64)
    if rec.shape != (rows,):
        raise ValueError(f"crps_bracket: the record must be [{rows}], got shape {rec.shape}")
    if e.shape not in ((B + 1,), (rows, B + 1)):
        raise ValueError(f"crps_bracket: edges must be [{B + 1}] or [{rows}][{B + 1}], got shape {e.shape}")
    e = np.broadcast_to(e, (rows, B + 1))
    lower, upper = np.full(c3.shape[:2], np.nan), np.full(c3.shape[:2], np.nan)
    for r in range(rows):
        y = float(rec[r])
        if y != y or not e[r, 0] <= y <= e[r, B]:
            continue
        ef, yf = [Fraction(v) for v in e[r].tolist()], Fraction(y)
        for g in range(c3.shape[1]):
            T = int(total[r, g])
            if T == 0 or below[r, g] != 0 or above[r, g] != 0:
                continue
            lo = hi = Fraction(0)
            C = 0
            for k, c in enumerate(c3[r, g].tolist()):
                a, b = Fraction(C, T), Fraction(C + c, T)      # C_k / T <= F <= C_{k+1} / T inside bin k
                C += c
                left = min(max(yf, ef[k]), ef[k + 1]) - ef[k]  # the part of the bin left of y
                right = (ef[k + 1] - ef[k]) - left
                lo += left * a * a + right * (1 - b) * (1 - b)
                hi += left * b * b + right * (1 - a) * (1 - a)
            lower[r, g], upper[r, g] = float(lo), float(hi)
    return {"lower": lower.reshape(shape), "upper": upper.reshape(shape)}


def moment_blocks(K: int, order: int) -> int:
    """Blocks per group of ``Ensemble.moment_sums``: K sums of order 1, the K (K + 1) / 2 pairs a <= b of order 2."""
    return K if order == 1 else K * (K + 1) // 2


def moment_finish(blocks, divisor, n_terms: int) -> np.ndarray:
    """rscm_gpu_moment_finish: ``blocks[B][69]`` int64 (68 limbs in units of 2^(32 k - 1088) and a count of non-finite terms) over
    ``divisor`` (one int64, or one per block) as B doubles, each the exact quotient rounded once.  No device is needed."""
    blocks = np.ascontiguousarray(blocks, dtype=np.int64).reshape(-1, L.MOMENT_BLOCK)
    div = np.ascontiguousarray(np.broadcast_to(np.asarray(divisor, dtype=np.int64), (blocks.shape[0],)))
    out = np.empty(blocks.shape[0])
    i64 = C.POINTER(C.c_int64)
    L.check(L.load().rscm_gpu_moment_finish(blocks.ctypes.data_as(i64), blocks.shape[0], div.ctypes.data_as(i64), int(n_terms), L.dptr(out)))
    return out


def _moment_sums_args(what: str, order: int, center, center_shape, B: int):
    """For ``Ensemble.moment_sums`` and ``Ensemble.moment_rows_sums``: the checked ``center`` ``[*leading][values per record]`` of
    order 2 as a flat float64 array (``None`` at order 1), and the zeroed int64 output ``[*leading][2 + B * 69]``."""
    if order not in (1, 2):
        raise ValueError(f"{what}: order must be 1 or 2")
    c = None
    if order == 2:
        if center is None:
            raise ValueError(f"{what}: order 2 needs a center")
        c = np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(-1))
        if c.size != int(np.prod(center_shape)):
            raise ValueError(f"center: need {' x '.join(map(str, center_shape))} values, got {c.size}")
    return c, np.zeros(tuple(center_shape[:-1]) + (2 + B * L.MOMENT_BLOCK,), dtype=np.int64)


def _moment_sums_finish(sums, B: int, lead) -> np.ndarray:
    """``[*lead][B]`` doubles from (reduced) sums ``[*lead][2 + B * 69]``: every block over its record's W, in one call of
    rscm_gpu_moment_finish, which refuses a count outside [0, 2^31)."""
    sums = np.asarray(sums, dtype=np.int64).reshape(*lead, 2 + B * L.MOMENT_BLOCK)
    if sums.size == 0:
        return np.empty(sums.shape[:-1] + (B,))
    n = sums[..., 0]
    out = moment_finish(sums[..., 2:], np.repeat(sums[..., 1].reshape(-1), B), int(n.min() if n.min() < 0 else n.max()))
    return out.reshape(sums.shape[:-1] + (B,))


def moment_means(sums1, K: int, G: int) -> np.ndarray:
    """``mean[G][K]`` from the (reduced) order-1 sums ``[G][2 + K * 69]`` of ``Ensemble.moment_sums``."""
    return _moment_sums_finish(sums1, K, (G,))


def moments_dict(n, w, mean, cov, grouped: bool = True) -> Dict[str, np.ndarray]:
    """``{"count", "weight", "mean", "cov", "sd", "corr"}`` from ``n[G]``, ``w[G]``, ``mean[G][K]``, ``cov[G][K][K]``: ``sd_a =
    sqrt(cov_aa)``, ``corr_ab = cov_ab / (sd_a sd_b)`` for a < b, mirrored; the diagonal is exactly 1.0 where ``cov_aa > 0``, NaN
    otherwise.  Plain float64 numpy, the same on every rank.  Without ``grouped`` the group axis (of length 1) is dropped."""
    n, w = np.asarray(n, dtype=np.int64), np.asarray(w, dtype=np.int64)
    mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    K = mean.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.einsum("gaa->ga", cov)
        sd = np.sqrt(var)
        corr = np.empty_like(cov)
        for a in range(K):
            corr[:, a, a] = np.where(var[:, a] > 0.0, 1.0, np.nan)
            for b in range(a + 1, K):
                corr[:, a, b] = corr[:, b, a] = cov[:, a, b] / (sd[:, a] * sd[:, b])
    out = {"count": n, "weight": w, "mean": mean, "cov": cov, "sd": sd, "corr": corr}
    return out if grouped else {k: v[0] for k, v in out.items()}


def moments_result(sums1, sums2, K: int, G: int, grouped: bool = True) -> Dict[str, np.ndarray]:
    """Finishes the (reduced) sums of ``Ensemble.moment_sums`` -- ``sums1[G][2 + K * 69]`` of order 1 and ``sums2[G][2 + K (K + 1)
    / 2 * 69]`` of order 2 about ``moment_means(sums1, K, G)`` -- through rscm_gpu_moment_finish and forms ``moments_dict``."""
    B = moment_blocks(K, 2)
    sums2 = np.asarray(sums2, dtype=np.int64).reshape(G, 2 + B * L.MOMENT_BLOCK)
    tri = _moment_sums_finish(sums2, B, (G,))
    cov = np.empty((G, K, K))
    iu = np.triu_indices(K)          # row-major upper triangle: (0,0), (0,1), ..., (0,K-1), (1,1), ...
    cov[:, iu[0], iu[1]] = tri
    cov[:, iu[1], iu[0]] = tri
    return moments_dict(sums2[:, 0], sums2[:, 1], moment_means(sums1, K, G), cov, grouped)


def moment_rows_blocks(K: int, order: int) -> int:
    """Blocks per row and group of ``Ensemble.moment_rows_sums``: 1 + K sums of order 1, 1 + 2 K of order 2."""
    return 1 + K if order == 1 else 1 + 2 * K


def moment_rows_means(sums1, K: int, G: int) -> np.ndarray:
    """``mean[rows][G][1 + K]`` from the (reduced) order-1 sums of ``Ensemble.moment_rows_sums``: the centre of its order 2."""
    return _moment_sums_finish(sums1, 1 + K, (-1, G))


def moment_rows_dict(n, w, mean, second, grouped: bool = True) -> Dict[str, np.ndarray]:
    """The dict of ``Ensemble.moment_rows`` from ``n[rows][G]``, ``w[rows][G]``, ``mean[rows][G][1 + K]`` and ``second[rows][G][1 +
    2 K]``: ``sd = sqrt(var)``, ``corr = cov / (sd * sqrt(vec_var))`` (the rule of ``moments_dict``), ``slope = cov / vec_var``, one
    IEEE operation each on the finished values.  Plain float64 numpy, the same on every rank.  Without ``grouped`` the group axis
    (of length 1) is dropped."""
    n, w = np.asarray(n, dtype=np.int64), np.asarray(w, dtype=np.int64)
    mean, second = np.asarray(mean, dtype=np.float64), np.asarray(second, dtype=np.float64)
    K = mean.shape[-1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        var = second[..., 0]
        out = {"count": n, "weight": w, "mean": mean[..., 0], "var": var, "sd": np.sqrt(var)}
        if K:
            cov, vec_var = second[..., 1:1 + K], second[..., 1 + K:]
            out.update({"vec_mean": mean[..., 1:], "vec_var": vec_var, "cov": cov,
                        "corr": cov / (out["sd"][..., None] * np.sqrt(vec_var)), "slope": cov / vec_var})
    return out if grouped else {k: v[:, 0] for k, v in out.items()}


def moment_rows_result(sums1, sums2, K: int, G: int, grouped: bool = True) -> Dict[str, np.ndarray]:
    """Finishes the (reduced) sums of ``Ensemble.moment_rows_sums`` -- ``sums1[rows][G][2 + (1 + K) * 69]`` of order 1 and
    ``sums2[rows][G][2 + (1 + 2 K) * 69]`` of order 2 about ``moment_rows_means(sums1, K, G)`` -- through rscm_gpu_moment_finish and
    forms ``moment_rows_dict``."""
    sums2 = np.asarray(sums2, dtype=np.int64).reshape(-1, G, 2 + (1 + 2 * K) * L.MOMENT_BLOCK)
    return moment_rows_dict(sums2[:, :, 0], sums2[:, :, 1], moment_rows_means(sums1, K, G), _moment_sums_finish(sums2, 1 + 2 * K, (-1, G)), grouped)


def select_flags(weighted: bool, anomaly: bool, grouped: bool) -> int:
    return L.SELECT_WEIGHTED * bool(weighted) | L.SELECT_ANOMALY * bool(anomaly) | L.SELECT_GROUPED * bool(grouped)


def select_result(out: np.ndarray, cnt: np.ndarray, weighted: bool, grouped: bool) -> Dict[str, np.ndarray]:
    """The result dict of a select from the library's ``out[rows][G][n_q]`` and ``count[rows][G]``: group-major with ``grouped``,
    the group axis dropped without."""
    cnt = cnt.astype(np.int64)
    if grouped:
        out, cnt = np.ascontiguousarray(out.transpose(1, 0, 2)), np.ascontiguousarray(cnt.T)
    else:
        out, cnt = out[:, 0, :], cnt[:, 0]
    return {"weight" if weighted else "count": cnt, "quantiles": out}


def default_weight_bits(n_total: int) -> int:
    """The quantisation depth that keeps ``n_total`` weights of at most ``2**bits`` summing to at most 2^53."""
    n = int(n_total)
    if n <= 1:
        return 52
    return 53 - (n - 1).bit_length()   # ceil(log2(n)) for n >= 2


class QuantileSelect:
    """A staged select in flight on one ensemble (rscm_ens_select_*)::

        with ens.select(var, q) as s:
            while (buf := s.next_pass()) is not None:
                ... SUM-all-reduce buf (int64) over every shard ...
                s.commit()            # or s.commit(reduced_host_array)
            res = s.result()
    """

    def __init__(self, ens: Ensemble, var, q, t_begin: int, t_end: Optional[int], t_stride: int, weighted: bool = False,
                 anomaly: bool = False, vectors=None, grouped: bool = False):
        self.ens = ens
        self.q = np.atleast_1d(L.f64(q))
        self.weighted = bool(weighted)
        self.grouped = bool(grouped)
        self.n_groups = ens._n_groups(grouped)
        flags = select_flags(weighted, anomaly, grouped)
        if vectors is not None:                      # rscm_ens_select_begin_vectors: the vectors are the rows
            arr, self.rows = ens._vectors(vectors)
            L.check(ens._lib.rscm_ens_select_begin_vectors(ens._h, self.rows, arr, self.q.size, L.dptr(self.q), flags))
        else:
            t_end = ens.n_times if t_end is None else t_end
            self.rows = len(range(t_begin, t_end, t_stride)) if t_stride > 0 else 0
            L.check(ens._lib.rscm_ens_select_begin_ex(ens._h, ens._var(var), t_begin, t_end, t_stride, self.q.size, L.dptr(self.q), flags))
        self._open = True
        self._buf = None

    def next_pass(self) -> Optional[DeviceVector]:
        """This handle's int64 histograms of the next pass, in device memory, or ``None`` when no pass is left."""
        done, n = C.c_int32(0), C.c_int64(0)
        p = C.POINTER(C.c_int64)()
        L.check(self.ens._lib.rscm_ens_select_pass(self.ens._h, C.byref(done), C.byref(p), C.byref(n)))
        if done.value:
            self._buf = None
            return None
        self._buf = DeviceVector(C.cast(p, C.c_void_p).value, n.value, np.int64, self.ens)
        return self._buf

    def commit(self, reduced: Optional[np.ndarray] = None) -> None:
        """Move every target one digit on from the (reduced) buffer; ``reduced``: host sums to copy into it first."""
        if reduced is not None:
            r = np.ascontiguousarray(reduced, dtype=np.int64)
            if self._buf is None or r.size != self._buf.n:
                raise ValueError("reduced histograms do not match this pass's buffer")
            L.check(L.load().rscm_gpu_copy_to_device(self.ens.device, C.c_void_p(self._buf.ptr), r.ctypes.data_as(C.c_void_p), r.nbytes))
        L.check(self.ens._lib.rscm_ens_select_commit(self.ens._h))

    def result(self) -> Dict[str, np.ndarray]:
        out, cnt = np.empty((self.rows, self.n_groups, self.q.size)), np.empty((self.rows, self.n_groups))
        L.check(self.ens._lib.rscm_ens_select_result(self.ens._h, L.dptr(out), L.dptr(cnt)))
        return select_result(out, cnt, self.weighted, self.grouped)

    def close(self) -> None:
        if self._open:
            self._open = False
            L.check(self.ens._lib.rscm_ens_select_end(self.ens._h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _PinnedOwner:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            L.load().rscm_gpu_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def run_lockstep(ensembles: Sequence["Ensemble"], step_end: Optional[int] = None, *, sync: bool = True) -> None:
    """``Model::run`` over linked ensembles: every step, each ensemble in the order given advances by
    one step (``rscm_ens_run_lockstep``); all must stand at the same time index and share a stream."""
    first = ensembles[0]
    end = first.n_times - 1 if step_end is None else step_end
    arr = (C.c_void_p * len(ensembles))(*[e._h.value for e in ensembles])
    L.check(first._lib.rscm_ens_run_lockstep(arr, len(ensembles), first.time_index, end))
    if sync:
        first.sync()


def pinned_empty(shape, dtype=np.float64) -> np.ndarray:
    """numpy array over page-locked host memory (hipHostMalloc); freed with the array."""
    lib = L.load()
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = C.c_void_p()
    L.check(lib.rscm_gpu_host_alloc(max(n, 1), C.byref(p)))
    owner = _PinnedOwner(p.value)
    buf = (C.c_char * max(n, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    arr = arr.view(_PinnedArray)
    arr._owner = owner
    return arr


class _PinnedArray(np.ndarray):
    """ndarray that keeps its page-locked allocation alive."""

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


def selftest_div(num, den, device: int = 0):
    """(ref, fast, used_fast) of num/den on the device; see rscm_gpu_selftest_div."""
    lib = L.load()
    a, b = L.f64(num).ravel(), L.f64(den).ravel()
    ref, fast = np.empty_like(a), np.empty_like(a)
    used = np.empty(a.size, dtype=np.uint8)
    L.check(lib.rscm_gpu_selftest_div(device, a.size, L.dptr(a), L.dptr(b), L.dptr(ref),
                                      L.dptr(fast), L.bptr(used)))
    return ref, fast, used


def selftest_pair_div(num, den, num_lo: int = -902, device: int = 0):
    """(ieee, plain, verdict, variant) of num/den on the device; see rscm_gpu_selftest_pair_div."""
    lib = L.load()
    a, b = L.f64(num).ravel(), L.f64(den).ravel()
    ieee, plain, tried = np.empty_like(a), np.empty_like(a), np.empty_like(a)
    variant = np.empty(a.size, dtype=np.int32)
    L.check(lib.rscm_gpu_selftest_pair_div(device, a.size, num_lo, L.dptr(a), L.dptr(b), L.dptr(ieee), L.dptr(plain), L.dptr(tried),
                                           variant.ctypes.data_as(C.POINTER(C.c_int32))))
    return ieee, plain, tried, variant


def selftest_math(op: int, x, y=None):
    """out[i] of op 0 log_f64(x), 1 the device library's log, 2 its exp, 3 chem::pow_ratio(x, y), 4 guarded_rcp(x) on the current
    device; see rscm_gpu_selftest_math."""
    lib = L.load()
    a = L.f64(x).ravel()
    b = None if y is None else L.f64(y).ravel()
    if b is not None and b.size != a.size:
        raise ValueError(f"x has {a.size} elements, y {b.size}")
    out = np.empty_like(a)
    L.check(lib.rscm_gpu_selftest_math(int(op), a.size, L.dptr(a), None if b is None else L.dptr(b), L.dptr(out)))
    return out
