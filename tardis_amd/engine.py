"""Thin object wrapper over the C ABI (one Engine = one TardisMcContext = one GPU + one stream)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _lib
from . import state as st


class MonteCarloException(ValueError):
    """Mirror of tardis.transport.montecarlo.utils.MonteCarloException (utils.py:9)."""


class MacroAtomError(ValueError):
    """Mirror of tardis.transport.montecarlo.macro_atom.MacroAtomError (macro_atom.py:15)."""


class EventLogOverflow(RuntimeError):
    """The device pool of the full r-packet log was too small for the last call: rows were dropped.  ``rows_needed`` is the
    exact capacity (option ``event_log_capacity``) with which a re-run of the same call keeps every row."""

    def __init__(self, rows_needed: int, dropped: int):
        super().__init__(f"full r-packet log overflow: {dropped} of {rows_needed} rows dropped; re-run with "
                         f"event_log_capacity={rows_needed}")
        self.rows_needed, self.dropped = int(rows_needed), int(dropped)


class VPacketLogOverflow(RuntimeError):
    """The device v-packet log was too small for the last call: entries were dropped.  ``entries_needed`` is the capacity (option
    ``vpacket_log_capacity``) with which a re-run of the same call keeps every entry."""

    def __init__(self, entries_needed: int):
        super().__init__(f"v-packet log overflow: re-run with vpacket_log_capacity={entries_needed}")
        self.entries_needed = int(entries_needed)


class Engine:
    def __init__(self, device_id: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        rc = self._L.tardis_mc_create(int(device_id), C.byref(h))
        if rc != 0:
            msg = self._L.tardis_mc_last_error(None).decode()
            raise _lib.EngineUnavailable(f"tardis_mc_create(device {device_id}) failed ({rc}): {msg}")
        self._h = h
        self._keep = {}
        self.n_packets = self.n_shells = self.n_lines = self.n_grid = 0
        self.n_levels = 0  # macro-atom levels (blocks) of the resident opacity tables
        self.n_transitions = 0
        self.line_data = None        # the object whose data set_line_data() uploaded (None after every set_opacity / run)
        self.plasma_data = None      # ... and set_plasma_data() (None after every set_opacity / set_line_data / run)
        self.nlte_data = None        # ... and set_nlte_data() (None after whatever drops the plasma data)
        self.nlte_collision_data = None  # ... and set_nlte_collision_data() (None after whatever drops the NLTE data)
        self.ionization_options = None   # ... and set_ionization_options(): (helium_treatment, helium_element, delta_treatment); None after whatever drops the plasma data
        self.continuum_data = None       # ... and set_continuum_data(); None after whatever drops the plasma data
        self.bf_t_electrons = None       # ... and set_bf_estimators(); None after whatever drops the continuum data
        self.n_continua = self.n_continuum_points = 0
        self.n_helium_levels = 0
        self.n_nlte_collision_pairs = 0
        self.n_nlte_levels = 0
        self.n_plasma_levels = self.n_ions = 0
        self.opacity_generation = 0  # bumped whenever the resident opacity tables are replaced (lazy DeviceOpacityState views check it)
        self._vpk_log = False
        self._n_v = 0
        self.packets_generation = 0  # bumped whenever the resident packets are replaced (lazy host views check it)
        self.results_generation = 0  # bumped by every propagate() that succeeded
        # bumped by everything that changes the resident estimators: propagate, reset_estimators, allreduce_estimators
        # (lazy views of a resident run check it: a later reset / all-reduce must not be read as that run's estimators)
        self.estimators_generation = 0
        # the opacity object whose tables are in HBM (None: unknown) -- residency is a property of the ENGINE, which several
        # solvers and the non-resident entry point may share (MCTransportSolverHIP reuses the upload only against this)
        self.resident_opacity = None
        self.resident_geometry = None  # likewise (geometry object, time_explosion) of the last set_geometry()
        self.options = {}  # options set through set_option (name -> last value accepted by the library)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.tardis_mc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what, packet_index=-1):
        if rc == 0:
            return
        msg = self._L.tardis_mc_last_error(self._h).decode()
        exc = None
        if rc == _abi.ERR_MONTECARLO:
            exc = MonteCarloException("nu difference is less than 0.0")
        elif rc == _abi.ERR_MACRO_ATOM:
            exc = MacroAtomError("MacroAtom ran out of the block. This should not happen as the sum of "
                                 "probabilities is normalized to 1 and the probability_event should be less than 1")
        elif rc == _abi.ERR_UNSUPPORTED:
            exc = NotImplementedError("macro-atom transition type outside classic mode (continuum processes)")
        if exc is not None:
            exc.packet_index = packet_index  # lowest failing packet index (the reference aborts on the first one)
            exc.code = rc
            raise exc
        exc = RuntimeError(f"{what} failed ({rc}): {msg}")
        exc.code = rc  # (the TARDIS_MC_ERR_* value, _abi.ERR_*)
        raise exc

    # -- staged API
    def set_option(self, name: str, value: int):
        self._check(self._L.tardis_mc_set_option(self._h, name.encode(), int(value)), f"set_option({name})")
        self.options[name] = int(value)

    def set_geometry(self, geometry, time_explosion=None):
        m = _abi.marshal_geometry(geometry, time_explosion)
        self.resident_geometry = None
        self._check(self._L.tardis_mc_set_geometry(self._h, m.ref()), "set_geometry")
        if int(m.struct.n_shells) != self.n_shells:
            self.bf_t_electrons = None  # (the library drops the estimator setup with the shell count)
        self.n_shells = int(m.struct.n_shells)
        self.resident_geometry = (geometry, float(m.struct.time_explosion))

    def set_opacity(self, opacity_state):
        m = _abi.marshal_opacity(opacity_state)
        self.resident_opacity = None  # (a failed upload leaves the tables undefined)
        self.line_data = None
        self.plasma_data = None
        self.nlte_data = None
        self.nlte_collision_data = None
        self.ionization_options = None
        self.continuum_data = None
        self.bf_t_electrons = None
        self.opacity_generation += 1
        self._check(self._L.tardis_mc_set_opacity(self._h, m.ref()), "set_opacity")
        self.n_lines, self.n_shells = int(m.struct.n_lines), int(m.struct.n_shells)
        self.n_levels = max(0, int(m.struct.n_macro_block_edges) - 1)
        self.n_transitions = int(m.struct.n_transitions)
        self.resident_opacity = opacity_state

    def set_line_data(self, line_data):
        """The static line data of update_opacity() (`tardis_mc_set_line_data`), after set_opacity(): an object with f_lu,
        wavelength_cm, g_lower, g_upper, level_lower, level_upper [n_lines], n_levels, sobolev_coefficient and
        transition_probability_coef [n_transitions] (None in scatter mode), e.g. ``synthetic.make_line_data``.  A later
        set_opacity() drops them."""
        m = _abi.marshal_line_data(line_data, self.n_transitions)
        self.line_data = None
        self.plasma_data = None
        self.nlte_data = None
        self.nlte_collision_data = None
        self.ionization_options = None
        self.continuum_data = None
        self.bf_t_electrons = None
        self._check(self._L.tardis_mc_set_line_data(self._h, m.ref()), "set_line_data")
        self.line_data = line_data

    def update_opacity(self, level_number_density, electron_density=None, j_blues_mode=_abi.J_BLUES_DILUTE_BLACKBODY, *,
                       t_radiative=None, dilution_factor=None, time_of_simulation=0.0, volume=None, w_epsilon=1e-10,
                       detailed_optical_window=False) -> None:
        """tau_sobolev, beta_sobolev, the stimulated-emission factor, j_blues and the transition probabilities of the next iteration,
        computed on the device from ``level_number_density`` [n_levels, n_shells] (`tardis_mc_update_opacity`): the resident tables
        are replaced as set_opacity() would replace them, nothing of [n_lines, n_shells] crosses the bus.  ``j_blues_mode`` 0: dilute
        black body of ``t_radiative`` / ``dilution_factor``; 1: the detailed j_blues radiation_field() returns for
        (``time_of_simulation``, ``volume``, ``w_epsilon``, ``detailed_optical_window``), after propagate().  ``electron_density``
        None keeps the resident values.  No host object describes the new tables: ``resident_opacity`` becomes None until the
        caller names one (transport.MCTransportSolverHIP.update_opacity does)."""
        m = _abi.marshal_opacity_update(level_number_density, self.n_shells, electron_density, j_blues_mode, t_radiative,
                                        dilution_factor, time_of_simulation, volume, w_epsilon, detailed_optical_window)
        self.resident_opacity = None
        self.opacity_generation += 1
        self._check(self._L.tardis_mc_update_opacity(self._h, m.ref()), "update_opacity")

    def get_opacity(self, tau_sobolev=True, transition_probabilities=True, beta_sobolev=False, stimulated_emission_factor=False,
                    j_blues=False) -> dict:
        """The resident opacity tables, downloaded line-major as set_opacity() takes them (`tardis_mc_get_opacity`): a dict of the
        arrays asked for -- tau_sobolev, beta_sobolev, stimulated_emission_factor, j_blues [n_lines, n_shells],
        transition_probabilities [n_transitions, n_shells].  The last three exist only after update_opacity()."""
        S, L, T = self.n_shells, self.n_lines, self.n_transitions
        want = (("tau_sobolev", tau_sobolev, L), ("transition_probabilities", transition_probabilities, T),
                ("beta_sobolev", beta_sobolev, L), ("stimulated_emission_factor", stimulated_emission_factor, L), ("j_blues", j_blues, L))
        out = {name: np.empty((rows, S)) for name, on, rows in want if on}
        self._check(self._L.tardis_mc_get_opacity(self._h, *(out[name].ctypes.data if on else None for name, on, _ in want)),
                    "get_opacity")
        return out

    def last_opacity_update_ms(self) -> dict:
        """Device time (ms) of the stages of the last update_opacity(): {"line_ms" (population transpose, detailed j_blues, line
        kernel), "block_ms" (block kernels), "derive_ms" (the tables derived from the probabilities)}."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._L.tardis_mc_last_opacity_update_ms(self._h, C.byref(a), C.byref(b), C.byref(c)), "last_opacity_update_ms")
        return {"line_ms": a.value, "block_ms": b.value, "derive_ms": c.value}

    @staticmethod
    def opacity_update_path(rows: int) -> str:
        """The form of update_opacity()'s block kernel for a macro-atom block of ``rows`` transitions: "lane" (one lane per
        (block, shell)) or "row" (a 16-lane row per (block, shell)); csrc/opacity_update_plan.hpp."""
        return ("lane", "row")[int(_lib.lib().tardis_mc_opacity_update_path(int(rows)))]

    def mean_opacity(self, t_radiative, bin_size=10, want_expansion=False) -> dict:
        """The expansion opacity of the resident tau_sobolev in frequency bins of ``bin_size`` lines, its Planck and Rosseland means
        with electron scattering and the optical depths summed from the surface inward (`tardis_mc_mean_opacity`; the header states
        the arithmetic): {"kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland": [n_shells]; "bins_low", "delta_nu":
        [n_bins]; "bin_size", "n_bins"}, with ``want_expansion`` also "kappa_expansion" [n_bins, n_shells].  Needs set_geometry() and
        an opacity state (set_opacity / update_opacity / update_plasma); changes nothing resident.  A ``bin_size`` at which a bin
        has width 0 is refused (RuntimeError, ``code`` ERR_INVALID_ARGUMENT): see ``mean_opacity_bins``."""
        m, L = int(bin_size), self.n_lines
        n_bins = (L + m - L % m) // m if m >= 1 and L >= 1 else 1
        # (before any set_geometry / set_opacity the library refuses the call: the request only has to be well formed)
        n_shells = self.n_shells or (1 if t_radiative is None else np.size(t_radiative))
        q = _abi.marshal_mean_opacity(t_radiative, m, n_shells, n_bins, want_expansion)
        self._check(self._L.tardis_mc_mean_opacity(self._h, q.ref()), "mean_opacity")
        out = dict(q.out)
        out["bin_size"], out["n_bins"] = m, n_bins
        return out

    def last_mean_opacity_ms(self) -> dict:
        """Device time (ms) of the stages of the last mean_opacity(): {"bin_ms" (bin kernel), "reduce_ms" (shell reduction and the
        final kernel)}."""
        a, b = C.c_double(), C.c_double()
        self._check(self._L.tardis_mc_last_mean_opacity_ms(self._h, C.byref(a), C.byref(b)), "last_mean_opacity_ms")
        return {"bin_ms": a.value, "reduce_ms": b.value}

    @staticmethod
    def mean_opacity_bins(line_list_nu, bin_size: int) -> tuple[int, int]:
        """The bin layout of mean_opacity() for a descending line list (`tardis_mc_mean_opacity_bins`, host only): (n_bins, -1), or
        (error code < 0, first bin of width 0 or -1) where the library refuses the size; ``mean_opacity_bins_error()`` has the text."""
        nu = np.ascontiguousarray(line_list_nu, dtype=np.float64)
        first = C.c_int64(-1)
        n = _lib.lib().tardis_mc_mean_opacity_bins(len(nu), nu.ctypes.data, int(bin_size), C.byref(first))
        return int(n), int(first.value)

    @staticmethod
    def mean_opacity_bins_error() -> str:
        """The message of the last refusal of mean_opacity_bins() on this thread."""
        return _lib.lib().tardis_mc_last_error(None).decode()

    @staticmethod
    def mean_opacity_path(n_bins: int) -> str:
        """The form of mean_opacity()'s shell reduction for ``n_bins`` bins: "lane" (one lane per shell) or "row" (a wave per shell,
        four 16-lane rows); csrc/mean_opacity_plan.hpp."""
        return ("lane", "row")[int(_lib.lib().tardis_mc_mean_opacity_path(int(n_bins)))]

    def set_plasma_data(self, plasma_data):
        """The static plasma data of update_plasma() (`tardis_mc_set_plasma_data`), after set_line_data(): an object with the
        fields of ``synthetic.PlasmaData`` -- the levels' energies, weights and metastable flags, the ion and element edges, the ions'
        charges, ionization energies and zeta rows, the elements' number densities per shell, chi_0 and link_t_rad_t_electron.  A
        later set_opacity() or set_line_data() drops them."""
        m = _abi.marshal_plasma_data(plasma_data)
        self.plasma_data = None
        self.nlte_data = None
        self.nlte_collision_data = None
        self.ionization_options = None
        self.continuum_data = None
        self.bf_t_electrons = None
        self._check(self._L.tardis_mc_set_plasma_data(self._h, m.ref()), "set_plasma_data")
        self.n_plasma_levels, self.n_ions = int(m.struct.n_levels), int(m.struct.n_ions)
        self.plasma_data = plasma_data

    def update_plasma(self, t_radiative, dilution_factor, ionization="nebular", excitation="dilute-lte",
                      j_blues_mode=_abi.J_BLUES_DILUTE_BLACKBODY, *, time_of_simulation=0.0, volume=None, w_epsilon=1e-10,
                      detailed_optical_window=False) -> None:
        """The plasma of the next iteration solved on the device from two [n_shells] vectors (`tardis_mc_update_plasma`): level and
        ion populations and the electron density of ``ionization`` "nebular" / "lte" and ``excitation`` "dilute-lte" / "lte", and on
        them everything update_opacity() computes -- as if the populations and the solved electron density had been passed to it, but
        nothing of [levels, shells] crosses the bus.  ``j_blues_mode`` and the keywords as in update_opacity().  A failed solve
        (RuntimeError with ``code`` ERR_STATE: NaN, or no convergence within option "plasma_max_iterations") leaves the resident
        tables as they were."""
        try:
            modes = _abi.IONIZATION_MODES[ionization], _abi.EXCITATION_MODES[excitation]
        except KeyError as e:
            raise ValueError(f"unknown ionization / excitation mode {e.args[0]!r}") from None
        m = _abi.marshal_plasma_update(t_radiative, dilution_factor, self.n_shells, modes[0], modes[1], j_blues_mode,
                                       time_of_simulation, volume, w_epsilon, detailed_optical_window)
        previous = self.resident_opacity
        self.resident_opacity = None
        rc = self._L.tardis_mc_update_plasma(self._h, m.ref())
        if rc in (_abi.ERR_STATE, _abi.ERR_INVALID_ARGUMENT, _abi.ERR_UNSUPPORTED):
            self.resident_opacity = previous  # (refused before any table was touched)
        else:
            self.opacity_generation += 1
        self._check(rc, "update_plasma")

    def get_plasma(self, level_number_density=True, ion_number_density=True, partition_function=True, electron_density=True) -> dict:
        """The plasma the last update_plasma() solved (`tardis_mc_get_plasma`): a dict of the arrays asked for --
        level_number_density [n_levels, n_shells], ion_number_density, partition_function [n_ions, n_shells], electron_density
        [n_shells] -- and "iterations", the passes of the electron-density iteration."""
        S = self.n_shells
        want = (("level_number_density", level_number_density, (self.n_plasma_levels, S)), ("ion_number_density", ion_number_density, (self.n_ions, S)),
                ("partition_function", partition_function, (self.n_ions, S)), ("electron_density", electron_density, (S,)))
        out = {name: np.empty(shape) for name, on, shape in want if on}
        it = C.c_int32(-1)
        self._check(self._L.tardis_mc_get_plasma(self._h, *(out[name].ctypes.data if on else None for name, on, _ in want), C.byref(it)),
                    "get_plasma")
        out["iterations"] = int(it.value)
        return out

    def last_plasma_update_ms(self) -> dict:
        """Device time (ms) of the stages of the last update_plasma(): {"boltzmann_ms", "partition_ms", "ionization_ms",
        "population_ms"}, then the three of last_opacity_update_ms()."""
        v = [C.c_double() for _ in range(4)]
        self._check(self._L.tardis_mc_last_plasma_update_ms(self._h, *(C.byref(x) for x in v)), "last_plasma_update_ms")
        out = dict(zip(("boltzmann_ms", "partition_ms", "ionization_ms", "population_ms"), (x.value for x in v)))
        out.update(self.last_opacity_update_ms())
        return out

    def set_ionization_options(self, helium_treatment=None, helium_element=None, delta_treatment=None):
        """The switches of update_plasma()'s nebular ionisation (`tardis_mc_set_ionization_options`), after set_plasma_data():
        ``helium_treatment`` None or "recomb-nlte" (what ``plasma.helium_treatment`` is to a configuration), ``helium_element`` the
        element row that is helium -- None: the row where ``plasma_data.atomic_number == 2``, ValueError when there is none --, and
        ``delta_treatment`` None or the number that replaces the radiation-field correction.  All three None clears the options;
        whatever drops the plasma data drops them too, set_nlte_data() does not."""
        self.ionization_options = None
        if helium_treatment is None and delta_treatment is None:
            self._check(self._L.tardis_mc_set_ionization_options(self._h, None), "set_ionization_options")
            return
        m = _abi.marshal_ionization_options(helium_treatment, helium_element, delta_treatment, self.plasma_data)
        self._check(self._L.tardis_mc_set_ionization_options(self._h, m.ref()), "set_ionization_options")
        self.n_helium_levels = 0
        if m.struct.helium_treatment:
            pd, e = self.plasma_data, int(m.struct.helium_element)
            a, b = int(pd.element_ion_edge[e]), int(pd.element_ion_edge[e + 1])
            self.n_helium_levels = int(pd.ion_level_edge[b]) - int(pd.ion_level_edge[a])
        self.ionization_options = (helium_treatment, helium_element, delta_treatment)

    def get_helium(self, relative_population=True, level_number_density=True) -> dict:
        """Helium of the last update_plasma() with helium_treatment (`tardis_mc_get_helium`): relative_population (the populations
        relative to the He II ground level before the electron density enters) and level_number_density (those of the pass whose
        electron density was handed out), [helium levels, n_shells] each."""
        want = (("relative_population", relative_population), ("level_number_density", level_number_density))
        out = {name: np.empty((self.n_helium_levels, self.n_shells)) for name, on in want if on}
        self._check(self._L.tardis_mc_get_helium(self._h, *(out[name].ctypes.data if on else None for name, on in want)), "get_helium")
        return out

    def last_helium_ms(self) -> dict:
        """Device time (ms) of the relative-population kernel of the last update_plasma() with helium_treatment: {"relative_ms"}."""
        a = C.c_double()
        self._check(self._L.tardis_mc_last_helium_ms(self._h, C.byref(a)), "last_helium_ms")
        return {"relative_ms": a.value}

    def set_continuum_data(self, continuum_data):
        """The photo-ionisation cross-sections of update_plasma()'s continuum stage (`tardis_mc_set_continuum_data`), after
        set_plasma_data(): an object with the fields of ``synthetic.ContinuumData`` -- the levels that have a cross-section table,
        the block edges (photo_ion_block_references) and nu / x_sect of every point; what ``plasma.continuum_interaction.species``
        is to a configuration.  From then on every successful update_plasma() leaves the rate coefficients, chi_bf and the free-free
        factor of its populations resident (get_continuum_rates, get_continuum_opacity, continuum_opacity); nothing else of the
        update changes.  None removes the data; whatever drops the plasma data drops them too, set_nlte_data(),
        set_nlte_collision_data() and set_ionization_options() do not."""
        self.continuum_data = None
        self.bf_t_electrons = None
        if continuum_data is None:
            self._check(self._L.tardis_mc_set_continuum_data(self._h, None), "set_continuum_data")
            return
        m = _abi.marshal_continuum_data(continuum_data)
        self._check(self._L.tardis_mc_set_continuum_data(self._h, m.ref()), "set_continuum_data")
        self.n_continua, self.n_continuum_points = int(m.struct.n_continua), int(m.struct.n_points)
        self.continuum_data = continuum_data

    @staticmethod
    def check_continuum_data(continuum_data, plasma_data) -> tuple[int, str]:
        """What set_continuum_data() would say to ``continuum_data`` on ``plasma_data`` (`tardis_mc_check_continuum_data`, host
        only): (0, "") or (ERR_INVALID_ARGUMENT, the message naming the rule and the first offending index)."""
        m = _abi.marshal_continuum_data(continuum_data)
        ion_edge = np.ascontiguousarray(plasma_data.ion_level_edge, dtype=np.int64)
        elem_edge = np.ascontiguousarray(plasma_data.element_ion_edge, dtype=np.int64)
        L = _lib.lib()
        rc = L.tardis_mc_check_continuum_data(m.ref(), int(ion_edge[-1]), len(ion_edge) - 1, ion_edge.ctypes.data, elem_edge.ctypes.data)
        return int(rc), ("" if rc == 0 else L.tardis_mc_last_error(None).decode())

    CONTINUUM_RATES = ("phi_ik", "alpha_sp", "gamma", "alpha_stim", "gamma_corr", "coll_ion", "coll_recomb")

    def get_continuum_rates(self) -> dict:
        """The rate coefficients of the last update_plasma() with continuum data (`tardis_mc_get_continuum_rates`): phi_ik,
        alpha_sp, gamma, alpha_stim, gamma_corr, coll_ion and coll_recomb, [n_continua, n_shells] each."""
        out = {name: np.empty((self.n_continua, self.n_shells)) for name in self.CONTINUUM_RATES}
        self._check(self._L.tardis_mc_get_continuum_rates(self._h, *(out[name].ctypes.data for name in self.CONTINUUM_RATES)), "get_continuum_rates")
        return out

    def get_continuum_opacity(self, chi_bf=True) -> dict:
        """The opacity tables of the last update_plasma() with continuum data (`tardis_mc_get_continuum_opacity`): chi_bf
        [n_points, n_shells] (unless ``chi_bf`` is False), ff_opacity_factor and t_electrons [n_shells], and the counts
        n_negative_chi_bf / n_negative_gamma_corr of the values the stage clamped to 0.0 (the reference raises on the first)."""
        S = self.n_shells
        out = {"ff_opacity_factor": np.empty(S), "t_electrons": np.empty(S)}
        if chi_bf:
            out["chi_bf"] = np.empty((self.n_continuum_points, S))
        a, b = C.c_int64(-1), C.c_int64(-1)
        self._check(self._L.tardis_mc_get_continuum_opacity(self._h, out["chi_bf"].ctypes.data if chi_bf else None, out["ff_opacity_factor"].ctypes.data,
                                                            out["t_electrons"].ctypes.data, C.byref(a), C.byref(b)), "get_continuum_opacity")
        out["n_negative_chi_bf"], out["n_negative_gamma_corr"] = int(a.value), int(b.value)
        return out

    def continuum_opacity(self, nu, shell, each=False) -> dict:
        """The continuum opacity of the resident tables at the pairs (nu[q], shell[q]) (`tardis_mc_continuum_opacity`; ``shell``
        may be one number for all): chi_bf_tot, chi_ff and n_current [n]; with ``each`` also chi_bf_each and x_sect_each
        [n, n_continua], 0.0 where a continuum is not current at the frequency."""
        q = _abi.marshal_continuum_query(nu, shell, self.n_continua, each)
        self._check(self._L.tardis_mc_continuum_opacity(self._h, q.ref()), "continuum_opacity")
        return dict(q.out)

    def last_continuum_ms(self) -> dict:
        """Device time (ms) of the continuum stage of the last update_plasma(): {"thermal_ms" (t_e, the free-free factor, the
        thermal Boltzmann factors and partition functions), "points_ms", "rates_ms", "opacity_ms" (chi_bf)}; none of it is in
        last_plasma_update_ms()."""
        v = [C.c_double() for _ in range(4)]
        self._check(self._L.tardis_mc_last_continuum_ms(self._h, *(C.byref(x) for x in v)), "last_continuum_ms")
        return dict(zip(("thermal_ms", "points_ms", "rates_ms", "opacity_ms"), (x.value for x in v)))

    COOLING_RATES = ("c_fb_sp", "cool_rate_fb", "cool_rate_coll_ion")
    COOLING_SHELL_RATES = ("cool_rate_ff", "cool_rate_adiabatic", "cool_rate_total")

    def get_cooling_rates(self) -> dict:
        """The cooling rates of the last update_plasma() with continuum data (`tardis_mc_get_cooling_rates`): c_fb_sp, cool_rate_fb
        and cool_rate_coll_ion [n_continua, n_shells]; cool_rate_ff, cool_rate_adiabatic and cool_rate_total [n_shells].
        Collisional-excitation cooling is not part of the total."""
        out = {name: np.empty((self.n_continua, self.n_shells)) for name in self.COOLING_RATES}
        out.update({name: np.empty(self.n_shells) for name in self.COOLING_SHELL_RATES})
        self._check(self._L.tardis_mc_get_cooling_rates(self._h, *(out[name].ctypes.data for name in self.COOLING_RATES + self.COOLING_SHELL_RATES)),
                    "get_cooling_rates")
        return out

    def get_kpacket_tables(self, fb_emission_cdf=True) -> dict:
        """The tables the k-packet samplers read (`tardis_mc_get_kpacket_tables`): fb_emission_cdf [n_points, n_shells] (unless
        ``fb_emission_cdf`` is False), k_cdf [2 + 2 n_continua, n_shells] -- its entries: ff, adiabatic, the continua's free-bound
        rates, their collisional-ionisation rates -- and n_degenerate_fb_cdf, the number of (continuum, shell) whose emission integral
        was not positive and finite (their CDF is 0.0 up to the last point and 1.0 there; the reference produces NaN)."""
        S = self.n_shells
        out = {"k_cdf": np.empty((2 + 2 * self.n_continua, S))}
        if fb_emission_cdf:
            out["fb_emission_cdf"] = np.empty((self.n_continuum_points, S))
        a = C.c_int64(-1)
        self._check(self._L.tardis_mc_get_kpacket_tables(self._h, out["fb_emission_cdf"].ctypes.data if fb_emission_cdf else None, out["k_cdf"].ctypes.data,
                                                         C.byref(a)), "get_kpacket_tables")
        out["n_degenerate_fb_cdf"] = int(a.value)
        return out

    def kpacket_sample(self, shell, z_process, z_nu, force_kind=None, force_continuum=None) -> dict:
        """What the k-packets (shell[q], z_process[q], z_nu[q]) turn into on the resident tables (`tardis_mc_kpacket_sample`; ``shell``
        may be one number for all): kind (0 ff, 1 adiabatic, 2 fb, 3 coll_ion; ``_abi.KPACKET_KINDS``), continuum (-1 for kinds 0 and 1)
        and nu [n] -- the free-free or free-bound frequency at z_nu for kinds 0 and 2, 0.0 for kinds 1 and 3.  Both z lie in [0, 1).
        ``force_kind`` / ``force_continuum`` (one number or [n], -1: sample) set the kind and, for kinds 2 and 3, the continuum."""
        q = _abi.marshal_kpacket_query(shell, z_process, z_nu, force_kind, force_continuum)
        self._check(self._L.tardis_mc_kpacket_sample(self._h, q.ref()), "kpacket_sample")
        return dict(q.out)

    def last_cooling_ms(self) -> dict:
        """Device time (ms) of the cooling sub-stage of the last update_plasma(), per kernel: {"points_ms" (the two integrands),
        "blocks_ms" (c_fb_sp, the rate tables, the emission CDFs), "table_ms" (the shell rates and k_cdf)}; none of it is in
        last_continuum_ms() or last_plasma_update_ms()."""
        v = [C.c_double() for _ in range(3)]
        self._check(self._L.tardis_mc_last_cooling_ms(self._h, *(C.byref(x) for x in v)), "last_cooling_ms")
        return dict(zip(("points_ms", "blocks_ms", "table_ms"), (x.value for x in v)))

    # -- photo-ionisation and heating estimators from the transport (option "bf_estimators")
    BF_ESTIMATORS = ("photo_ion", "stim_recomb", "bf_heating", "stim_recomb_cooling")

    def set_bf_estimators(self, t_electrons):
        """The electron temperatures [n_shells] of the photo-ionisation estimators (`tardis_mc_set_bf_estimators`), after
        set_continuum_data(): installs them and the zeroed tables.  With option "bf_estimators" 1 every propagate() then logs one
        record per move of positive length and adds it to the tables (get_bf_estimators).  None switches the estimators off.
        Whatever drops the continuum data drops this."""
        self.bf_t_electrons = None
        if t_electrons is None:
            self._check(self._L.tardis_mc_set_bf_estimators(self._h, None), "set_bf_estimators")
            return
        m = _abi.marshal_bf_estimator_setup(t_electrons, self.n_shells)
        self._check(self._L.tardis_mc_set_bf_estimators(self._h, m.ref()), "set_bf_estimators")
        self.bf_t_electrons = m.keep[0]

    @staticmethod
    def check_bf_estimator_setup(t_electrons) -> tuple[int, str]:
        """What set_bf_estimators() would say to ``t_electrons`` (`tardis_mc_check_bf_estimator_setup`, host only): (0, "") or
        (ERR_INVALID_ARGUMENT, the message naming the first offending index)."""
        t = np.ascontiguousarray(t_electrons, dtype=np.float64)
        m = _abi.marshal_bf_estimator_setup(t, len(t))
        L = _lib.lib()
        rc = L.tardis_mc_check_bf_estimator_setup(m.ref(), len(t))
        return int(rc), ("" if rc == 0 else L.tardis_mc_last_error(None).decode())

    def get_bf_estimators(self) -> dict:
        """The estimator tables (`tardis_mc_get_bf_estimators`): photo_ion, stim_recomb, bf_heating, stim_recomb_cooling (float64)
        and statistics (int64), [n_continua, n_shells] each, with n_records / n_dropped since the last reset_estimators().  With
        dropped records the RuntimeError (``code`` ERR_STATE) carries the two counts as ``n_records`` / ``n_dropped``."""
        shape = (self.n_continua, self.n_shells)
        out = {name: np.empty(shape) for name in self.BF_ESTIMATORS}
        out["statistics"] = np.empty(shape, dtype=np.int64)
        a, b = C.c_int64(-1), C.c_int64(-1)
        rc = self._L.tardis_mc_get_bf_estimators(self._h, *(out[name].ctypes.data for name in self.BF_ESTIMATORS + ("statistics",)), C.byref(a), C.byref(b))
        try:
            self._check(rc, "get_bf_estimators")
        except RuntimeError as e:
            e.n_records, e.n_dropped = int(a.value), int(b.value)
            raise
        out["n_records"], out["n_dropped"] = int(a.value), int(b.value)
        return out

    def get_segment_log(self) -> dict:
        """Tests: the segment records of the last propagate() (`tardis_mc_get_segment_log`; needs option "segment_log_keep"), in no
        particular order: {"nu", "ed" (float64), "shell" (int64)}."""
        n = C.c_int64(-1)
        self._check(self._L.tardis_mc_get_segment_log(self._h, None, None, None, 0, C.byref(n)), "get_segment_log")
        out = {"nu": np.empty(n.value), "ed": np.empty(n.value), "shell": np.empty(n.value, dtype=np.int64)}
        if n.value:
            self._check(self._L.tardis_mc_get_segment_log(self._h, out["nu"].ctypes.data, out["ed"].ctypes.data, out["shell"].ctypes.data, n.value, C.byref(n)),
                        "get_segment_log")
        return out

    def debug_bf_accumulate(self, nu, ed, shell) -> None:
        """Tests: the accumulate pass alone on caller-supplied records (`tardis_mc_debug_bf_accumulate`), into the resident tables."""
        nu = np.ascontiguousarray(nu, dtype=np.float64)
        ed = np.ascontiguousarray(ed, dtype=np.float64)
        shell = np.ascontiguousarray(np.broadcast_to(np.asarray(shell, dtype=np.int64), nu.shape))
        if ed.shape != nu.shape or nu.ndim != 1:
            raise ValueError("nu, ed and shell are one-dimensional and of one length")
        self._check(self._L.tardis_mc_debug_bf_accumulate(self._h, len(nu), nu.ctypes.data, ed.ctypes.data, shell.ctypes.data), "debug_bf_accumulate")
        self.estimators_generation += 1

    def last_bf_estimator_ms(self) -> dict:
        """Device time (ms) of the last accumulate pass: {"group_ms" (the record slots grouped by shell), "accumulate_ms"}; none of
        it is in any other timer."""
        v = [C.c_double() for _ in range(2)]
        self._check(self._L.tardis_mc_last_bf_estimator_ms(self._h, *(C.byref(x) for x in v)), "last_bf_estimator_ms")
        return dict(zip(("group_ms", "accumulate_ms"), (x.value for x in v)))

    def bf_estimator_rates(self, time_of_simulation, volume) -> dict:
        """gamma_est and stim_est [n_continua, n_shells] from the resident tables (`tardis_mc_bf_estimator_rates`): photo_ion and
        stim_recomb times 1 / ((time_of_simulation volume[s]) h).  They stay resident -- through reset_estimators() too -- for
        update_plasma() under option "continuum_field" 1."""
        volume = np.ascontiguousarray(volume, dtype=np.float64)
        if volume.shape != (self.n_shells,):
            raise ValueError("volume must be [n_shells]")
        self._check(self._L.tardis_mc_bf_estimator_rates(self._h, float(time_of_simulation), volume.ctypes.data), "bf_estimator_rates")
        out = {name: np.empty((self.n_continua, self.n_shells)) for name in ("gamma_est", "stim_est")}
        self._check(self._L.tardis_mc_get_bf_estimator_rates(self._h, out["gamma_est"].ctypes.data, out["stim_est"].ctypes.data), "get_bf_estimator_rates")
        return out

    def set_nlte_data(self, nlte_data):
        """The NLTE species of update_plasma() (`tardis_mc_set_nlte_data`), after set_plasma_data(): an object with the fields of
        ``synthetic.NlteData`` -- the species' ions, their lines in the line list with A_ul, B_ul and B_lu, and the flags
        coronal_approximation and classical_nebular.  From then on update_plasma() replaces the species' level Boltzmann factors by
        those of the statistical equilibrium of the radiative rates; a failed solve is a RuntimeError with ``code`` ERR_STATE that
        leaves the resident tables as they were.  None removes the data; whatever drops the plasma data drops them too."""
        self.nlte_data = None
        self.nlte_collision_data = None
        if nlte_data is None:
            self._check(self._L.tardis_mc_set_nlte_data(self._h, None), "set_nlte_data")
            return
        m = _abi.marshal_nlte_data(nlte_data)
        self._check(self._L.tardis_mc_set_nlte_data(self._h, m.ref()), "set_nlte_data")
        edge = np.asarray(self.plasma_data.ion_level_edge)
        self.n_nlte_levels = int(np.sum(np.diff(edge)[np.asarray(nlte_data.species_ion, dtype=np.int64)]))
        self.nlte_data = nlte_data

    def get_nlte(self, level_boltzmann_factor=True, relative_populations=True) -> dict:
        """What the NLTE stage of the last update_plasma() produced (`tardis_mc_get_nlte`): level_boltzmann_factor
        [n_levels, n_shells] (every level; the NLTE species' rows replaced) and relative_populations, the solutions x of the
        species one after the other, [sum of their levels, n_shells]."""
        S = self.n_shells
        want = (("level_boltzmann_factor", level_boltzmann_factor, self.n_plasma_levels), ("relative_populations", relative_populations, self.n_nlte_levels))
        out = {name: np.empty((rows, S)) for name, on, rows in want if on}
        self._check(self._L.tardis_mc_get_nlte(self._h, *(out[name].ctypes.data if on else None for name, on, _ in want)), "get_nlte")
        return out

    def set_nlte_collision_data(self, collision_data):
        """The collisional rates of the NLTE species (`tardis_mc_set_nlte_collision_data`), after set_nlte_data(): an object with the
        fields of ``synthetic.NlteCollisionData`` -- a temperature grid and, per species, pairs of local levels with delta_e (kelvin),
        g_ratio and C_ul over the grid; what ``collision_data`` is to the atomic data.  From then on update_plasma() adds
        c_ul n_e / c_lu n_e of every pair to the species' rate matrices, n_e the electron density resident at entry to the call; an
        electron temperature outside the grid is a RuntimeError with ``code`` ERR_INVALID_ARGUMENT that leaves the state.  None removes
        the data; whatever drops the NLTE data (a new set_nlte_data() included) drops them too."""
        self.nlte_collision_data = None
        if collision_data is None:
            self._check(self._L.tardis_mc_set_nlte_collision_data(self._h, None), "set_nlte_collision_data")
            return
        m = _abi.marshal_nlte_collision_data(collision_data)
        self._check(self._L.tardis_mc_set_nlte_collision_data(self._h, m.ref()), "set_nlte_collision_data")
        self.n_nlte_collision_pairs = int(m.struct.n_pairs)
        self.nlte_collision_data = collision_data

    def get_nlte_collision_rates(self, c_ul=True, c_lu=True) -> dict:
        """c_ul and c_lu [n_pairs, n_shells] as the last update_plasma() formed them, before the product with the electron density
        (`tardis_mc_get_nlte_collision_rates`)."""
        want = (("c_ul", c_ul), ("c_lu", c_lu))
        out = {name: np.empty((self.n_nlte_collision_pairs, self.n_shells)) for name, on in want if on}
        self._check(self._L.tardis_mc_get_nlte_collision_rates(self._h, *(out[name].ctypes.data if on else None for name, on in want)),
                    "get_nlte_collision_rates")
        return out

    def last_nlte_ms(self) -> dict:
        """Device time (ms) of the NLTE stage of the last update_plasma(): {"assemble_ms" (the rates of the NLTE lines and, with
        collision data, of the pairs), "solve_ms" (the (species, shell) workgroups: matrix, elimination, substitution)}."""
        a, b = C.c_double(), C.c_double()
        self._check(self._L.tardis_mc_last_nlte_ms(self._h, C.byref(a), C.byref(b)), "last_nlte_ms")
        return {"assemble_ms": a.value, "solve_ms": b.value}

    @staticmethod
    def nlte_solve_path(levels: int) -> str:
        """The form of the NLTE solve kernel for a species of ``levels`` levels: "lds" or "global"; csrc/nlte_plan.hpp."""
        return ("lds", "global")[int(_lib.lib().tardis_mc_nlte_solve_path(int(levels)))]

    @staticmethod
    def nlte_solve_form(levels: int) -> str:
        """The form of the NLTE solve for a species of ``levels`` levels under the rule: "lds", "global" (one workgroup on a slab of
        HBM) or "blocked" (panels by one workgroup, the trailing update over the whole chip); csrc/nlte_plan.hpp.  Options
        ``nlte_lds_levels`` and ``nlte_blocked_levels`` move the two thresholds (measurements and tests); all forms give the same bits."""
        return _abi.NLTE_FORMS[int(_lib.lib().tardis_mc_nlte_solve_form(int(levels)))]

    @staticmethod
    def plasma_update_path(levels: int) -> str:
        """The form of update_plasma()'s partition kernel for an ion of ``levels`` levels: "lane" (one lane per (ion, shell)) or
        "row" (a 16-lane row per (ion, shell)); csrc/plasma_update_plan.hpp."""
        return ("lane", "row")[int(_lib.lib().tardis_mc_plasma_update_path(int(levels)))]

    def set_config(self, montecarlo_configuration, spectrum_frequency_grid, number_of_vpackets=None, sigma_thomson=None):
        m = _abi.marshal_config(montecarlo_configuration, spectrum_frequency_grid, number_of_vpackets, sigma_thomson)
        self._check(self._L.tardis_mc_set_config(self._h, m.ref()), "set_config")
        self.n_grid = int(m.struct.n_spectrum_grid)
        self._n_v = int(m.struct.number_of_vpackets)
        self._vpk_log = bool(m.struct.enable_vpacket_tracking) and self._n_v > 0

    def set_packets(self, packet_collection):
        m = _abi.marshal_packets(packet_collection)
        self._check(self._L.tardis_mc_set_packets(self._h, m.ref()), "set_packets")
        self.n_packets = int(m.struct.n_packets)
        self.packets_generation += 1

    def reset_estimators(self):
        self.estimators_generation += 1
        self._check(self._L.tardis_mc_reset_estimators(self._h), "reset_estimators")

    def propagate(self):
        # (whatever happens, the previous run's results are gone; the counters a view compares with only become valid --
        # equal to the view's -- for views created AFTER a successful call)
        self.results_generation += 1
        self.estimators_generation += 1
        self._check(self._L.tardis_mc_propagate(self._h), "propagate")
        self.results_generation += 1
        self.estimators_generation += 1

    def synchronize(self):
        self._check(self._L.tardis_mc_synchronize(self._h), "synchronize")

    def progress(self) -> tuple[int, int]:
        """(packets handed to the propagation kernel so far, packets of the call) of the running -- or the last -- propagate().
        Meant to be polled from another thread while propagate() blocks (tardis_mc_progress reads one device word on its own stream)."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._L.tardis_mc_progress(self._h, C.byref(a), C.byref(b)), "progress")
        return int(a.value), int(b.value)

    def last_propagate_ms(self) -> float:
        v = C.c_double()
        self._check(self._L.tardis_mc_last_propagate_ms(self._h, C.byref(v)), "last_propagate_ms")
        return v.value

    def last_kernel_times(self) -> dict:
        """Device time (ms) of the seeding and propagation launches of the last propagate(), and the launch count."""
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        self._check(self._L.tardis_mc_last_kernel_times(self._h, C.byref(a), C.byref(b), C.byref(n)), "last_kernel_times")
        e = C.c_double()
        self._check(self._L.tardis_mc_last_estimator_ms(self._h, C.byref(e)), "last_estimator_ms")
        return {"seed_ms": a.value, "propagate_ms": b.value, "launches": n.value, "estimator_ms": e.value}

    def last_compactions(self) -> int:
        """How often the last propagate() packed the live lanes of its drain into fewer waves (option drain_compact)."""
        return int(self._L.tardis_mc_last_compactions(self._h))

    def last_tracker_defer(self) -> int:
        """How the last propagate() kept the last-interaction tracker (option ``tracker_defer``): 1 one record per packet, written when
        the packet ends; 0 a record per interaction; -1 another kernel than variant 3 without v-packets, or no tracker."""
        return int(self._L.tardis_mc_last_tracker_defer(self._h))

    KERNEL_TABLES = ("lane", "group", "wave")
    # the fields of a key, in the order of the row's template arguments (include/tardis_mc.h, tardis_mc_kernel_table_row)
    KERNEL_KEY_FIELDS = {"lane": ("FULL", "VPK", "TRACK", "FT", "VLI"),
                         "group": ("FULL", "TRACK", "G", "BLOCK", "OCC", "VPK", "WIDE", "VLI"),
                         "wave": ("FULL", "TRACK", "G", "VPK", "LS", "XWALK", "WPE", "NT", "SL", "FT", "WIDE", "VLI")}

    @staticmethod
    def kernel_table(table: str) -> list:
        """The rows of a table of compiled propagation kernels -- ``table`` "lane", "group" or "wave" -- as tuples of the rows' template
        arguments, in the order of ``KERNEL_KEY_FIELDS[table]`` (`tardis_mc_kernel_table_row`; needs no GPU)."""
        L, t = _lib.lib(), Engine.KERNEL_TABLES.index(table)
        key = (C.c_int * 12)()
        n = L.tardis_mc_kernel_table_row(t, -1, key)
        if n < 0:
            raise RuntimeError(f"tardis_mc_kernel_table_row({table}) failed ({n})")
        width = len(Engine.KERNEL_KEY_FIELDS[table])
        rows = []
        for r in range(n):
            L.tardis_mc_kernel_table_row(t, r, key)
            rows.append(tuple(key[:width]))
        return rows

    def last_kernel_key(self):
        """The kernel-table row the last propagate() launched: ("lane" | "group" | "wave", key as in kernel_table()), or (None, ()) when
        it looked no kernel up (`tardis_mc_last_kernel_key`)."""
        t, key = C.c_int(-1), (C.c_int * 12)()
        self._check(self._L.tardis_mc_last_kernel_key(self._h, C.byref(t), key), "last_kernel_key")
        if t.value < 0:
            return None, ()
        table = self.KERNEL_TABLES[t.value]
        return table, tuple(key[:len(self.KERNEL_KEY_FIELDS[table])])

    def last_variant(self) -> int:
        """Propagation kernel of the last propagate(): 0 lane, 1 group, 2 wave + group sweeps, 3 wave + lane sweeps,
        4 wave + volley queue (v-packets traced by vpacket_trace_kernel between its launches)."""
        return int(self._L.tardis_mc_last_variant(self._h))

    def last_sweep_skip(self) -> int:
        """Whether the lane sweeps of the last propagate() cleared whole 8-line blocks on the coarse prefix-sum table (option
        ``sweep_skip``): 1 or 0."""
        return int(self._L.tardis_mc_last_sweep_skip(self._h))

    def last_table_offsets(self) -> int:
        """Width of the table row offsets of the last propagate()'s kernel (option ``table_offsets``): 32 or 64 (variant 0
        always 64); -1 before the first call."""
        return int(self._L.tardis_mc_last_table_offsets(self._h))

    def get_event_log(self) -> st.FullTrackers:
        """The full r-packet log of the last propagate() (option ``track_full``), as ``state.FullTrackers``.  Raises
        ``EventLogOverflow`` when the device pool dropped rows (re-run with ``event_log_capacity`` = its ``rows_needed``)."""
        probe = _abi.TardisMcEventLog()
        offsets = np.zeros(self.n_packets + 1, dtype=np.int64)
        probe.offsets = _abi._ip(offsets)
        self._check(self._L.tardis_mc_get_event_log(self._h, C.byref(probe)), "get_event_log")
        if probe.dropped:
            raise EventLogOverflow(probe.count, probe.dropped)
        n = int(probe.count)
        cols = {f: np.empty(n) for f in _abi._EV_F64}
        cols.update({f: np.empty(n, dtype=np.int64) for f in _abi._EV_I64})
        log = _abi.TardisMcEventLog()
        log.capacity = n
        for f in _abi._EV_F64:
            setattr(log, f, _abi._dp(cols[f]))
        for f in _abi._EV_I64:
            setattr(log, f, _abi._ip(cols[f]))
        self._check(self._L.tardis_mc_get_event_log(self._h, C.byref(log)), "get_event_log")
        return st.FullTrackers(offsets, cols)

    def get_vpacket_log(self) -> st.VPacketCollection:
        """The v-packet log of the last propagate() (ENABLE_VPACKET_TRACKING), consolidated on the device (`tardis_mc_get_vpacket_log`): a
        ``state.VPacketCollection`` in packet order, then spawn order, plus ``offsets`` ([n_packets + 1]: packet p's entries are
        [offsets[p], offsets[p + 1])) and ``source_packet``.  After a call with the option ``vpacket_last_interaction`` the six
        ``last_interaction_*`` fields hold the spawning r-packet's last interaction (launch volley: -1 / NaN), otherwise the reference's
        -99 placeholders.  Raises ``VPacketLogOverflow`` when the device log dropped entries."""
        probe = _abi.TardisMcVpacketLog()
        self._check(self._L.tardis_mc_get_vpacket_log(self._h, C.byref(probe)), "get_vpacket_log")
        n = int(probe.count)
        vt = st.VPacketCollection(-1, None, None, None, self._n_v, n)
        vt.offsets = np.zeros(self.n_packets + 1, dtype=np.int64)
        vt.source_packet = np.empty(n, dtype=np.int64)
        log = _abi.TardisMcVpacketLog()
        log.capacity = n
        log.offsets, log.source_packet = _abi._ip(vt.offsets), _abi._ip(vt.source_packet)
        f64, i64 = _abi._VL_F64, _abi._VL_I64
        if not self.options.get("vpacket_last_interaction", 0):
            f64, i64 = f64[:4], ()
        for f in f64:
            setattr(log, f, _abi._dp(getattr(vt, f)))
        for f in i64:
            setattr(log, f, _abi._ip(getattr(vt, f)))
        vt.offsets[-1] = -1  # (the library writes no column when the device log overflowed)
        self._check(self._L.tardis_mc_get_vpacket_log(self._h, C.byref(log)), "get_vpacket_log")
        if vt.offsets[-1] != n:
            raise VPacketLogOverflow(n)
        return vt

    def get_results(self, output_nus=None, output_energies=None, track_last_interaction=True,
                    want_line_estimators=True, vpacket_log_capacity=None, want_packet_outputs=True, trackers=None,
                    track_full=False) -> _abi.ResultBuffers:
        """Copy results out.  Every part is optional: per-packet outputs (`want_packet_outputs`), the last-interaction
        trackers, the [L,S] line estimators -- whatever is not asked for stays on the device (the resident outer-iteration
        path reads the spectrum and the radiation field through packet_spectrum() / radiation_field() instead)."""
        # (`trackers`: the caller's own LastInteractionTrackers -- the library writes straight into its arrays instead of into fresh ones that
        # the caller would then copy: 1.1 GB allocated, touched and copied once more per 1e7 packets otherwise)
        if not track_last_interaction:
            trackers = None
        elif not (isinstance(trackers, st.LastInteractionTrackers) and len(trackers) == self.n_packets):
            trackers = st.LastInteractionTrackers(self.n_packets)
        cap = 0
        if self._vpk_log:
            cap = int(vpacket_log_capacity if vpacket_log_capacity is not None else self.n_packets * self._n_v * 64)
        res = _abi.ResultBuffers(self.n_packets, self.n_shells, self.n_lines, self.n_grid, output_nus, output_energies,
                                 trackers, cap, want_line_estimators, want_packet_outputs)
        rc = self._L.tardis_mc_get_results(self._h, res.ref())
        self._check(rc, "get_results", int(res.struct.first_error_packet))
        # (track_full: the full r-packet log of the call too -- it must have run with the option track_full)
        res.full_trackers = self.get_event_log() if track_full else None
        return res

    def stream_results(self, output_nus=None, output_energies=None, trackers=None) -> None:
        """Register the host arrays the NEXT propagate call may fill while it runs (`tardis_mc_stream_results`): a long call is several
        launches, and the per-packet results of the packets a launch has finished are copied beside the following launch instead of
        after the last one.  get_results() on the same arrays then sends only what is missing; on other arrays it copies everything.
        No arguments: disarm."""
        if output_nus is None and output_energies is None and trackers is None:
            self._stream_keep = None
            self._check(self._L.tardis_mc_stream_results(self._h, None), "stream_results")
            return
        if isinstance(trackers, st.LastInteractionTrackers) and len(trackers) != self.n_packets:
            raise ValueError("trackers must hold n_packets entries")
        res = _abi.ResultBuffers(self.n_packets, 0, 0, 0, output_nus, output_energies, trackers, 0, False, output_nus is not None)
        self._stream_keep = res  # (the arrays stay alive until the call that fills them is over)
        self._check(self._L.tardis_mc_stream_results(self._h, res.ref()), "stream_results")

    def streamed_packets(self) -> tuple[int, int]:
        """(packets whose results the last propagate call copied out while it ran, how many of them get_results sends again)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.tardis_mc_streamed_packets(self._h, C.byref(a), C.byref(b)), "streamed_packets")
        return int(a.value), int(b.value)

    def run(self, packet_collection, geometry, time_explosion, opacity_state, montecarlo_configuration, spectrum_frequency_grid,
            number_of_vpackets=None, track_last_interaction=True, vpacket_log_capacity=None,
            track_full=False) -> _abi.ResultBuffers:
        """The one-shot form of the boundary, `tardis_mc_run` (include/tardis_mc.h): geometry, opacity, configuration and packets in,
        one propagation, results out -- the call a ctypes binding inside `run_classic` makes when nothing is to stay resident
        (modes/classic/solver.py:223-234).  `vpacket_log_capacity`: entries of the caller's v-packet log arrays for THIS call (None:
        sized like get_results does; the library restores the context's own setting when the call returns, however it ends).
        `track_full`: also the full r-packet log, as ``res.full_trackers`` (state.FullTrackers)."""
        mp = _abi.marshal_packets(packet_collection)
        mg = _abi.marshal_geometry(geometry, time_explosion)
        mo = _abi.marshal_opacity(opacity_state)
        mc = _abi.marshal_config(montecarlo_configuration, spectrum_frequency_grid, number_of_vpackets)
        P, S, L = int(mp.struct.n_packets), int(mg.struct.n_shells), int(mo.struct.n_lines)
        n_v = int(mc.struct.number_of_vpackets)
        log = bool(mc.struct.enable_vpacket_tracking) and n_v > 0
        cap = (int(vpacket_log_capacity) if vpacket_log_capacity is not None else P * n_v * 64) if log else 0
        trackers = st.LastInteractionTrackers(P) if track_last_interaction else None
        res = _abi.ResultBuffers(P, S, L, int(mc.struct.n_spectrum_grid), None, None, trackers, cap)
        self.resident_opacity = None
        self.resident_geometry = None
        self.line_data = None
        self.plasma_data = None
        self.nlte_data = None
        self.nlte_collision_data = None
        self.ionization_options = None
        self.continuum_data = None
        self.bf_t_electrons = None
        self.opacity_generation += 1
        self.results_generation += 1
        self.estimators_generation += 1
        self.packets_generation += 1
        prev_full = self.options.get("track_full", 0)
        self.set_option("track_full", int(bool(track_full)))
        try:
            rc = self._L.tardis_mc_run(self._h, mp.ref(), mg.ref(), mo.ref(), mc.ref(), res.ref())
        finally:
            self.set_option("track_full", prev_full)
        self.n_packets, self.n_shells, self.n_lines, self.n_grid = P, S, L, int(mc.struct.n_spectrum_grid)
        self.n_levels = max(0, int(mo.struct.n_macro_block_edges) - 1)
        self.n_transitions = int(mo.struct.n_transitions)
        self._n_v, self._vpk_log = n_v, log
        self._check(rc, "run", int(res.struct.first_error_packet))
        res.full_trackers = self.get_event_log() if track_full else None
        self.resident_opacity = opacity_state
        self.results_generation += 1
        self.estimators_generation += 1
        return res

    def create_blackbody_packets(self, n_packets: int, radius: float, temperature: float, base_seed: int = 23111963,
                                 seed_offset: int = 0, *, first: int = 0, count: int | None = None,
                                 max_seed_val: int = 2**32 - 1, l_samples: int = 1000, time_explosion: float | None = None) -> None:
        """BlackBodySimpleSource.create_packets on the device (packet_source/base.py:195-253): the packets
        np.random.default_rng(base_seed + seed_offset) would have produced, slice [first, first+count), left resident
        as this engine's packet inputs.  With a ``time_explosion`` it is BlackBodySimpleSourceRelativistic, the source of a
        full-relativity run: beta = radius / time_explosion / c shifts the directions and scales the energies."""
        count = n_packets - first if count is None else count
        st = (C.c_uint64 * 4)()
        self._check(self._L.tardis_mc_pcg64_seed(int(base_seed + seed_offset), st), "pcg64_seed")
        l_array = np.cumsum(np.arange(1, l_samples, dtype=np.float64) ** -4)  # black_body.py:174
        if time_explosion is None:
            self._check(self._L.tardis_mc_create_blackbody_packets(self._h, int(n_packets), int(first), int(count), float(radius),
                                                                   float(temperature), st, int(max_seed_val),
                                                                   l_array.ctypes.data, len(l_array)), "create_blackbody_packets")
        else:
            self._check(self._L.tardis_mc_create_blackbody_packets_relativistic(
                self._h, int(n_packets), int(first), int(count), float(radius), float(temperature), float(time_explosion), st,
                int(max_seed_val), l_array.ctypes.data, len(l_array)), "create_blackbody_packets_relativistic")
        self.n_packets = int(count)
        self.packets_generation += 1

    def get_packets(self) -> dict:
        n = self.n_packets
        out = {k: np.empty(n) for k in ("initial_radii", "initial_nus", "initial_mus", "initial_energies")}
        out["packet_seeds"] = np.empty(n, dtype=np.int64)
        self._check(self._L.tardis_mc_get_packets(self._h, *(out[k].ctypes.data for k in
                                                             ("initial_radii", "initial_nus", "initial_mus", "initial_energies",
                                                              "packet_seeds"))), "get_packets")
        return out

    def packet_spectrum(self, time_of_simulation: float, luminosity_nu_start: float = 0.0,
                        luminosity_nu_end: float = float("inf")) -> dict:
        """Real-packet spectrum and filtered luminosities computed on the device from the resident packet outputs
        (what SpectrumSolver.montecarlo_emitted/reabsorbed_luminosity and calculate_filtered_luminosity return)."""
        B = self.n_grid - 1
        he, hr = np.zeros(B), np.zeros(B)
        le, lr = C.c_double(), C.c_double()
        self._check(self._L.tardis_mc_packet_spectrum(self._h, float(time_of_simulation), float(luminosity_nu_start),
                                                      float(luminosity_nu_end), he.ctypes.data, hr.ctypes.data,
                                                      C.byref(le), C.byref(lr)), "packet_spectrum")
        return {"montecarlo_emitted_luminosity": he, "montecarlo_reabsorbed_luminosity": hr,
                "emitted_luminosity": le.value, "reabsorbed_luminosity": lr.value}

    def packet_decomposition(self, time_of_simulation: float, line_class, n_classes: int | None = None, nu_start: float = 0.0,
                             nu_end: float = float("inf"), *, _virtual: bool = False) -> dict:
        """The emitted spectrum decomposed by last interaction, reduced on the device from the per-packet results of the last
        propagate() (`tardis_mc_packet_decomposition`; it must have run with track_last_interaction on): what SDEC, the
        last-interaction-velocity histogram and LastLineInteraction compute from the tracker's dataframe.  ``line_class``: [n_lines]
        integers in [0, C), the caller's grouping of the lines (``spectrum.species_classes``); C = ``n_classes``, or
        ``line_class.max() + 1``.  Returns {"emission", "absorption": (C, B), "no_interaction", "electron_scatter": (B,),
        "shell_packets": (C + 1, S) -- row C electron scattering --, "line_emit_packets", "line_absorb_packets": (L,),
        "n_selected", "n_line", "n_electron_scatter", "n_no_interaction"}, B the bins of the spectrum grid; definitions in
        include/tardis_mc.h.  No per-packet array leaves the device."""
        cls = np.ascontiguousarray(line_class, dtype=np.int64)
        if cls.shape != (self.n_lines,):
            raise ValueError("line_class must have one entry per line")
        if n_classes is None:
            n_classes = int(cls.max()) + 1 if cls.size else 1
        Cn, B, S, L = int(n_classes), max(self.n_grid - 1, 0), self.n_shells, self.n_lines
        rows = max(Cn, 0)  # (a refused n_classes sizes nothing)
        out = {"emission": np.zeros((rows, B)), "absorption": np.zeros((rows, B)), "no_interaction": np.zeros(B),
               "electron_scatter": np.zeros(B), "shell_packets": np.zeros((rows + 1, S), dtype=np.int64),
               "line_emit_packets": np.zeros(L, dtype=np.int64), "line_absorb_packets": np.zeros(L, dtype=np.int64)}
        d = _abi.TardisMcDecomposition()
        d.n_classes, d.line_class = Cn, _abi._ip(cls)
        d.time_of_simulation, d.nu_start, d.nu_end = float(time_of_simulation), float(nu_start), float(nu_end)
        for k in ("emission", "absorption", "no_interaction", "electron_scatter"):
            setattr(d, k, _abi._dp(out[k]))
        for k in ("shell_packets", "line_emit_packets", "line_absorb_packets"):
            setattr(d, k, _abi._ip(out[k]))
        if _virtual:
            self._check(self._L.tardis_mc_vpacket_decomposition(self._h, C.byref(d)), "vpacket_decomposition")
        else:
            self._check(self._L.tardis_mc_packet_decomposition(self._h, C.byref(d)), "packet_decomposition")
        for k in ("n_selected", "n_line", "n_electron_scatter", "n_no_interaction"):
            out[k] = int(getattr(d, k))
        return out

    def vpacket_decomposition(self, time_of_simulation: float, line_class, n_classes: int | None = None, nu_start: float = 0.0,
                              nu_end: float = float("inf")) -> dict:
        """packet_decomposition() of the VIRTUAL spectrum (SDEC / LIV with ``packets_mode="virtual"``), reduced on the device from the
        consolidated v-packet log of the last propagate() (`tardis_mc_vpacket_decomposition`; the call must have run with v-packet
        tracking and the option ``vpacket_last_interaction``).  Same arguments, same dict; no per-v-packet array leaves the device."""
        return self.packet_decomposition(time_of_simulation, line_class, n_classes, nu_start, nu_end, _virtual=True)

    @staticmethod
    def decomposition_path(n_classes: int, n_bins: int, n_shells: int) -> str:
        """The accumulation path packet_decomposition() takes for this shape: "privatised" (per-workgroup copies in LDS) or
        "direct" (global atomics); csrc/decomposition_plan.hpp."""
        return ("privatised", "direct")[int(_lib.lib().tardis_mc_decomposition_path(int(n_classes), int(n_bins), int(n_shells)))]

    def radiation_field(self, time_of_simulation: float, volume, w_epsilon: float = 1e-10,
                        detailed_optical_window: bool = False, want_j_blues: bool = True) -> dict:
        """MCRadiationFieldPropertiesSolver.solve (estimators/mc_rad_field_solver.py:37-144) on the resident estimators."""
        volume = np.ascontiguousarray(volume, dtype=np.float64)
        if volume.shape != (self.n_shells,):
            raise ValueError("volume must have one entry per shell")
        t_rad, w = np.empty(self.n_shells), np.empty(self.n_shells)
        jb = np.empty((self.n_lines, self.n_shells)) if want_j_blues else None
        self._check(self._L.tardis_mc_radiation_field(self._h, float(time_of_simulation), volume.ctypes.data, float(w_epsilon),
                                                      int(detailed_optical_window), t_rad.ctypes.data, w.ctypes.data,
                                                      jb.ctypes.data if jb is not None else None), "radiation_field")
        return {"t_radiative": t_rad, "dilution_factor": w, "j_blues": jb}

    def last_counters(self) -> dict:
        out = (C.c_int64 * len(_abi.COUNTER_NAMES))()
        self._check(self._L.tardis_mc_last_counters(self._h, out), "last_counters")
        return dict(zip(_abi.COUNTER_NAMES, [int(v) for v in out]))

    def formal_integral(self, inner_temperature: float, frequencies, att_S_ul, Jred_lu, Jblue_lu, n_impact_parameters: int = 1000,
                        want_intensities: bool = False):
        """numba_formal_integral (spectrum/formal_integral/formal_integral_numba.py:375-560) on the resident geometry / opacity:
        returns (luminosity_densities, intensities_nu_p or None)."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64).ravel()
        freqs, att, jred, jblue = f(frequencies), f(att_S_ul), f(Jred_lu), f(Jblue_lu)
        n = self.n_shells * self.n_lines
        if att.size != n or jred.size != n or jblue.size != n:
            raise ValueError("att_S_ul / Jred_lu / Jblue_lu must have n_shells * n_lines entries (shell-major)")
        lum = np.empty(freqs.size)
        inten = np.empty((freqs.size, int(n_impact_parameters))) if want_intensities else None
        self._check(self._L.tardis_mc_formal_integral(self._h, float(inner_temperature), freqs.ctypes.data, freqs.size, att.ctypes.data,
                                                      jred.ctypes.data, jblue.ctypes.data, int(n_impact_parameters), lum.ctypes.data,
                                                      inten.ctypes.data if inten is not None else None), "formal_integral")
        return lum, inten

    def source_function(self, time_of_simulation: float, volume, wavelength_cm=None, want_arrays: bool = True):
        """make_source_function (spectrum/formal_integral/source_function.py) on the resident estimators and tables
        (`tardis_mc_source_function`): after propagate() and, multi-GPU, allreduce_estimators().  Leaves att_S_ul / Jred_lu / Jblue_lu in
        HBM for formal_integral_resident().  Returns {"att_S_ul", "Jred_lu", "Jblue_lu": [n_shells * n_lines] shell-major, "e_dot_u":
        [levels, n_shells]}, or None with ``want_arrays=False`` (nothing is downloaded)."""
        volume = np.ascontiguousarray(volume, dtype=np.float64)
        if volume.shape != (self.n_shells,):
            raise ValueError("volume must have one entry per shell")
        wave = None
        if wavelength_cm is not None:
            wave = np.ascontiguousarray(wavelength_cm, dtype=np.float64)
            if wave.shape != (self.n_lines,):
                raise ValueError("wavelength_cm must have one entry per line")
        out = None
        if want_arrays:
            n = self.n_shells * self.n_lines
            levels = self.n_levels
            out = {"att_S_ul": np.empty(n), "Jred_lu": np.empty(n), "Jblue_lu": np.empty(n),
                   "e_dot_u": np.empty((levels, self.n_shells)) if levels > 0 else None}
        ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self._L.tardis_mc_source_function(
            self._h, float(time_of_simulation), volume.ctypes.data, ptr(wave),
            *((ptr(out["att_S_ul"]), ptr(out["Jred_lu"]), ptr(out["Jblue_lu"]), ptr(out["e_dot_u"])) if out else (None,) * 4)),
            "source_function")
        return out

    def last_source_iterations(self) -> int:
        """Fixed-point iterations of the last source_function() solve: 0 for downbranch, -1 before the first call."""
        return int(self._L.tardis_mc_last_source_iterations(self._h))

    def formal_integral_resident(self, inner_temperature: float, frequencies, n_impact_parameters: int = 1000,
                                 want_intensities: bool = False):
        """formal_integral() on the arrays source_function() left in HBM (`tardis_mc_formal_integral_resident`): returns
        (luminosity_densities, intensities_nu_p or None)."""
        freqs = np.ascontiguousarray(frequencies, dtype=np.float64).ravel()
        lum = np.empty(freqs.size)
        inten = np.empty((freqs.size, int(n_impact_parameters))) if want_intensities else None
        self._check(self._L.tardis_mc_formal_integral_resident(self._h, float(inner_temperature), freqs.ctypes.data, freqs.size,
                                                               int(n_impact_parameters), lum.ctypes.data,
                                                               inten.ctypes.data if inten is not None else None),
                    "formal_integral_resident")
        return lum, inten

    def formal_integral_interpolated(self, interpolate_shells: int, inner_temperature: float, frequencies,
                                     n_impact_parameters: int = 1000, want_intensities: bool = False):
        """formal_integral_resident() with the reference's ``interpolate_shells`` (`tardis_mc_formal_integral_interpolated`): the
        arrays source_function() left in HBM are interpolated on the device onto ``interpolate_shells - 1`` equal shells
        (interpolate_integrator_quantities) and integrated there.  The engine's resident state is left as it was.  Returns
        (luminosity_densities, intensities_nu_p or None)."""
        freqs = np.ascontiguousarray(frequencies, dtype=np.float64).ravel()
        lum = np.empty(freqs.size)
        inten = np.empty((freqs.size, int(n_impact_parameters))) if want_intensities else None
        self._check(self._L.tardis_mc_formal_integral_interpolated(self._h, int(interpolate_shells), float(inner_temperature),
                                                                   freqs.ctypes.data, freqs.size, int(n_impact_parameters),
                                                                   lum.ctypes.data, inten.ctypes.data if inten is not None else None),
                    "formal_integral_interpolated")
        return lum, inten

    def interpolated_source(self, interpolate_shells: int) -> dict:
        """What formal_integral_interpolated() integrates (`tardis_mc_interpolated_source`), with S' = interpolate_shells - 1:
        {"r_inner", "r_outer", "electron_density": [S'], "tau_sobolev", "att_S_ul", "Jred_lu", "Jblue_lu": [S' * n_lines]
        shell-major, "e_dot_u": [levels, S']}."""
        Si = int(interpolate_shells) - 1
        if not 1 <= Si < 65536:  # (the library refuses it: nothing to size the arrays by)
            Si = 0
        n, levels = Si * self.n_lines, self.n_levels
        out = {k: np.empty(Si) for k in ("r_inner", "r_outer", "electron_density")}
        out.update({k: np.empty(n) for k in ("tau_sobolev", "att_S_ul", "Jred_lu", "Jblue_lu")})
        out["e_dot_u"] = np.empty((levels, Si)) if levels > 0 else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self._L.tardis_mc_interpolated_source(
            self._h, int(interpolate_shells), *(ptr(out[k]) for k in ("r_inner", "r_outer", "electron_density", "tau_sobolev",
                                                                      "att_S_ul", "Jred_lu", "Jblue_lu", "e_dot_u"))),
            "interpolated_source")
        return out

    # -- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * _abi.UNIQUE_ID_BYTES)()
        rc = _lib.lib().tardis_mc_comm_get_unique_id(buf)
        if rc != 0:
            raise RuntimeError(f"tardis_mc_comm_get_unique_id failed ({rc})")
        return bytes(buf)

    def comm_init(self, rank: int, world_size: int, unique_id: bytes):
        buf = (C.c_uint8 * _abi.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._L.tardis_mc_comm_init(self._h, rank, world_size, buf), "comm_init")

    def comm_check(self) -> int:
        """Self-check of the RCCL communicator: the one-element all-reduce of (rank + 1) came back as N (N + 1) / 2; returns N."""
        n = C.c_int(0)
        self._check(self._L.tardis_mc_comm_check(self._h, C.byref(n)), "comm_check")
        return int(n.value)

    def allreduce_estimators(self):
        self.estimators_generation += 1
        self._check(self._L.tardis_mc_allreduce_estimators(self._h), "allreduce_estimators")

    # -- diagnostics
    def debug_eval(self, op: int, x, y=None, n=None) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = int(x.size if n is None else n)
        out = np.empty(n)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            yp = y.ctypes.data
        self._check(self._L.tardis_mc_debug_eval(self._h, op, x.ctypes.data, yp, out.ctypes.data, n), "debug_eval")
        return out

    PREFIX_TABLES = ("tau_pfx", "tau_rowsum", "pn", "ct", "sk_rowsum", "sk_state")

    def debug_prefix_table(self, name: str) -> np.ndarray:
        """A resident prefix-sum table as the kernels read it (op 101 of `tardis_mc_debug_eval`, tests): "tau_pfx" [S, L + 1] and "tau_rowsum" [S]
        of the v-packet screening; "pn" [S, L + 1, 2] = {frequency slot, prefix sum}, "ct" [S * ceil(L / 8) + 16, 2] = {nu_last, p_end}, "sk_rowsum" [S]
        and "sk_state" = [margin, negative, padded row length] of the block skip.  Raises when no propagate call has built the table."""
        S, L = self.n_shells, self.n_lines
        shape = {"tau_pfx": (S, L + 1), "tau_rowsum": (S,), "pn": (S, L + 1, 2), "ct": (S * ((L + 7) // 8) + 16, 2), "sk_rowsum": (S,), "sk_state": (3,)}[name]
        out = self.debug_eval(101, [self.PREFIX_TABLES.index(name), 0], n=int(np.prod(shape)))
        return out.reshape(shape)

    def debug_nlte_solve(self, m, b):
        """The blocked form of the NLTE solve on dense systems (`tardis_mc_debug_nlte_solve`): m [systems, n, n], b [systems, n] ->
        (x [systems, n], status [systems]: 0, 1 + the step of a bad pivot, n + 1 for x[0] == 0, n + 2 for an x that is not finite)."""
        m, b = np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        if m.ndim != 3 or m.shape[1] != m.shape[2] or b.shape != m.shape[:2]:
            raise ValueError("debug_nlte_solve needs m [systems, n, n] and b [systems, n]")
        x, status = np.empty(b.shape), np.empty(b.shape[0], dtype=np.int32)
        self._check(self._L.tardis_mc_debug_nlte_solve(self._h, m.shape[1], m.shape[0], m.ctypes.data, b.ctypes.data, x.ctypes.data, status.ctypes.data),
                    "debug_nlte_solve")
        return x, status

    def debug_set_line_estimators(self, j_blue, edotlu):
        """Plants the line estimators source_function() reads (`tardis_mc_debug_set_line_estimators`, for tests): j_blue and edotlu
        [n_lines, n_shells] as get_results() returns them, after set_opacity() and set_config()."""
        jb, ed = np.ascontiguousarray(j_blue, dtype=np.float64), np.ascontiguousarray(edotlu, dtype=np.float64)
        if jb.shape != (self.n_lines, self.n_shells) or ed.shape != jb.shape:
            raise ValueError("debug_set_line_estimators needs j_blue and edotlu [n_lines, n_shells]")
        self._check(self._L.tardis_mc_debug_set_line_estimators(self._h, jb.ctypes.data, ed.ctypes.data), "debug_set_line_estimators")
        self.estimators_generation += 1

    def debug_microbench(self, which: int, n_doubles: int, iters: int, blocks: int) -> float:
        v = C.c_double()
        self._check(self._L.tardis_mc_debug_microbench(self._h, which, n_doubles, iters, blocks, C.byref(v)), "microbench")
        return v.value


def device_count() -> int:
    return int(_lib.lib().tardis_mc_device_count())
