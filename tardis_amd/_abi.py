"""ctypes mirror of include/tardis_mc.h (struct layouts + marshalling from the Python state objects).

Only interface definitions live here: no library is loaded by importing this module.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import state as st

ABI_VERSION = 2
UNIQUE_ID_BYTES = 128
N_COUNTERS = 8
COUNTER_NAMES = ("line_visits", "events", "macro_transitions", "vpacket_line_visits", "vpackets", "rng_draws",
                 "packets", "reserved")

ERR_INVALID_ARGUMENT, ERR_HIP, ERR_MONTECARLO, ERR_MACRO_ATOM, ERR_UNSUPPORTED, ERR_COMM, ERR_STATE = (
    -1, -2, -3, -4, -5, -6, -7)

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int64)


class TardisMcConfig(C.Structure):
    _fields_ = [
        ("enable_full_relativity", C.c_int32),
        ("line_interaction_type", C.c_int32),
        ("disable_line_scattering", C.c_int32),
        ("enable_vpacket_tracking", C.c_int32),
        ("number_of_vpackets", C.c_int64),
        ("survival_probability", C.c_double),
        ("vpacket_tau_russian", C.c_double),
        ("vpacket_spawn_start_frequency", C.c_double),
        ("vpacket_spawn_end_frequency", C.c_double),
        ("sigma_thomson", C.c_double),
        ("n_spectrum_grid", C.c_int64),
        ("spectrum_frequency_grid", _pd),
    ]


class TardisMcPackets(C.Structure):
    _fields_ = [
        ("n_packets", C.c_int64),
        ("initial_radii", _pd),
        ("initial_nus", _pd),
        ("initial_mus", _pd),
        ("initial_energies", _pd),
        ("packet_seeds", _pi),
    ]


class TardisMcGeometry(C.Structure):
    _fields_ = [
        ("n_shells", C.c_int64),
        ("r_inner", _pd),
        ("r_outer", _pd),
        ("time_explosion", C.c_double),
    ]


class TardisMcOpacity(C.Structure):
    _fields_ = [
        ("n_lines", C.c_int64),
        ("n_shells", C.c_int64),
        ("n_transitions", C.c_int64),
        ("n_macro_block_edges", C.c_int64),
        ("electron_density", _pd),
        ("line_list_nu", _pd),
        ("tau_sobolev", _pd),
        ("transition_probabilities", _pd),
        ("line2macro_level_upper", _pi),
        ("macro_block_edge_index", _pi),
        ("transition_type", _pi),
        ("destination_level_id", _pi),
        ("transition_line_id", _pi),
    ]


class TardisMcLineData(C.Structure):
    """Static line data of the opacity update (tardis_mc_set_line_data)."""
    _fields_ = [
        ("n_lines", C.c_int64),
        ("n_transitions", C.c_int64),
        ("n_levels", C.c_int64),
        ("f_lu", _pd),
        ("wavelength_cm", _pd),
        ("g_lower", _pd),
        ("g_upper", _pd),
        ("level_lower", _pi),
        ("level_upper", _pi),
        ("transition_probability_coef", _pd),
        ("sobolev_coefficient", C.c_double),
    ]


class TardisMcOpacityUpdate(C.Structure):
    """One iteration's inputs of tardis_mc_update_opacity."""
    _fields_ = [
        ("level_number_density", _pd),
        ("electron_density", _pd),
        ("j_blues_mode", C.c_int32),
        ("t_radiative", _pd),
        ("dilution_factor", _pd),
        ("time_of_simulation", C.c_double),
        ("volume", _pd),
        ("w_epsilon", C.c_double),
        ("detailed_optical_window", C.c_int32),
    ]


J_BLUES_DILUTE_BLACKBODY, J_BLUES_DETAILED = 0, 1


class TardisMcMeanOpacity(C.Structure):
    """Request of tardis_mc_mean_opacity: bin size and radiation temperatures in, host outputs (any may be NULL)."""
    _fields_ = [
        ("bin_size", C.c_int64),
        ("t_radiative", _pd),
        ("kappa_planck", _pd),
        ("kappa_rosseland", _pd),
        ("tau_planck", _pd),
        ("tau_rosseland", _pd),
        ("kappa_expansion", _pd),
        ("bins_low", _pd),
        ("delta_nu", _pd),
    ]


class TardisMcPlasmaData(C.Structure):
    """Static plasma data of the plasma update (tardis_mc_set_plasma_data)."""
    _fields_ = [
        ("n_levels", C.c_int64),
        ("n_ions", C.c_int64),
        ("n_elements", C.c_int64),
        ("n_shells", C.c_int64),
        ("n_zeta_temperatures", C.c_int64),
        ("level_energy", _pd),
        ("level_g", _pd),
        ("level_metastable", C.POINTER(C.c_int32)),
        ("ion_level_edge", _pi),
        ("element_ion_edge", _pi),
        ("ion_charge", _pd),
        ("ionization_energy", _pd),
        ("zeta_temperatures", _pd),
        ("zeta", _pd),
        ("number_density", _pd),
        ("chi_0", C.c_double),
        ("link_t_rad_t_electron", C.c_double),
    ]


class TardisMcPlasmaUpdate(C.Structure):
    """One iteration's inputs of tardis_mc_update_plasma."""
    _fields_ = [
        ("t_radiative", _pd),
        ("dilution_factor", _pd),
        ("ionization_mode", C.c_int32),
        ("excitation_mode", C.c_int32),
        ("j_blues_mode", C.c_int32),
        ("time_of_simulation", C.c_double),
        ("volume", _pd),
        ("w_epsilon", C.c_double),
        ("detailed_optical_window", C.c_int32),
    ]


# tardis_mc_nlte_solve_form: the forms of the NLTE solve; options "nlte_lds_levels" / "nlte_blocked_levels" move their thresholds
NLTE_FORMS = ("lds", "global", "blocked")


class TardisMcNlteData(C.Structure):
    """The NLTE species of the plasma update and their lines (tardis_mc_set_nlte_data)."""
    _fields_ = [
        ("n_species", C.c_int64),
        ("species_ion", _pi),
        ("n_nlte_lines", C.c_int64),
        ("species_line_edge", _pi),
        ("line_id", _pi),
        ("A_ul", _pd),
        ("B_ul", _pd),
        ("B_lu", _pd),
        ("coronal_approximation", C.c_int32),
        ("classical_nebular", C.c_int32),
    ]


class TardisMcNlteCollisionData(C.Structure):
    """The collision strengths of the NLTE species' level pairs (tardis_mc_set_nlte_collision_data)."""
    _fields_ = [
        ("n_species", C.c_int64),
        ("n_temperatures", C.c_int64),
        ("collision_temperatures", _pd),
        ("n_pairs", C.c_int64),
        ("species_pair_edge", _pi),
        ("level_lower", _pi),
        ("level_upper", _pi),
        ("delta_e", _pd),
        ("g_ratio", _pd),
        ("C_ul", _pd),
    ]


class TardisMcIonizationOptions(C.Structure):
    """The switches of the nebular ionisation stage (tardis_mc_set_ionization_options)."""
    _fields_ = [
        ("helium_treatment", C.c_int32),
        ("use_delta_treatment", C.c_int32),
        ("helium_element", C.c_int64),
        ("delta_treatment", C.c_double),
    ]


class TardisMcContinuumData(C.Structure):
    """The photo-ionisation cross-sections of the continuum stage (tardis_mc_set_continuum_data)."""
    _fields_ = [
        ("n_continua", C.c_int64),
        ("level", _pi),
        ("block_edge", _pi),
        ("n_points", C.c_int64),
        ("nu", _pd),
        ("x_sect", _pd),
    ]


class TardisMcBfEstimatorSetup(C.Structure):
    """The electron temperatures of the photo-ionisation estimators (tardis_mc_set_bf_estimators)."""
    _fields_ = [("t_electrons", _pd)]


class TardisMcContinuumQuery(C.Structure):
    """A batch of (frequency, shell) pairs and where their continuum opacities go (tardis_mc_continuum_opacity)."""
    _fields_ = [
        ("n", C.c_int64),
        ("nu", _pd),
        ("shell", _pi),
        ("chi_bf_tot", _pd),
        ("chi_ff", _pd),
        ("n_current", _pi),
        ("chi_bf_each", _pd),
        ("x_sect_each", _pd),
    ]


class TardisMcKpacketQuery(C.Structure):
    """A batch of k-packets and where their processes and frequencies go (tardis_mc_kpacket_sample)."""
    _fields_ = [
        ("n", C.c_int64),
        ("shell", _pi),
        ("z_process", _pd),
        ("z_nu", _pd),
        ("kind", _pi),
        ("continuum", _pi),
        ("nu", _pd),
        ("force_kind", _pi),
        ("force_continuum", _pi),
    ]


KPACKET_KINDS = {"ff": 0, "adiabatic": 1, "fb": 2, "coll_ion": 3}
IONIZATION_MODES = {"nebular": 0, "lte": 1}
EXCITATION_MODES = {"dilute-lte": 0, "lte": 1}
HELIUM_TREATMENTS = {None: 0, "none": 0, "recomb-nlte": 1}


_LI_F64 = ("li_radius", "li_nu", "li_energy", "li_before_nu", "li_before_mu", "li_before_energy", "li_after_nu",
           "li_after_mu", "li_after_energy")
_LI_I64 = ("li_shell_id", "li_interaction_type", "li_line_absorb_id", "li_line_emit_id", "li_interactions_count")


class TardisMcResult(C.Structure):
    _fields_ = (
        [(n, _pd) for n in ("output_nus", "output_energies", "j_estimator", "nu_bar_estimator", "j_blue_estimator",
                            "edotlu_estimator", "v_packets_energy_hist")]
        + [(n, _pd) for n in _LI_F64]
        + [(n, _pi) for n in _LI_I64]
        + [("vpacket_log_capacity", C.c_int64), ("vpacket_log_count", C.c_int64)]
        + [(n, _pd) for n in ("vpacket_nus", "vpacket_energies", "vpacket_initial_mus", "vpacket_initial_rs")]
        + [("counters", C.c_int64 * N_COUNTERS), ("first_error_packet", C.c_int64), ("error_code", C.c_int32),
           ("reserved", C.c_int32)]
    )


_EV_I64 = ("event_id", "interaction_type", "status", "shell_id", "after_shell_id", "line_absorb_id", "line_emit_id")
_EV_F64 = ("radius", "before_nu", "before_mu", "before_energy", "after_nu", "after_mu", "after_energy")


class TardisMcEventLog(C.Structure):
    """Full r-packet tracking: CSR offsets + packet-major columns (tardis_mc_get_event_log)."""
    _fields_ = (
        [("capacity", C.c_int64), ("count", C.c_int64), ("dropped", C.c_int64), ("offsets", _pi)]
        + [(n, _pi) for n in _EV_I64]
        + [(n, _pd) for n in _EV_F64]
    )


_VL_F64 = ("nus", "energies", "initial_mus", "initial_rs", "last_interaction_in_nu", "last_interaction_in_r")
_VL_I64 = ("last_interaction_type", "last_interaction_in_id", "last_interaction_out_id", "last_interaction_shell_id")


class TardisMcVpacketLog(C.Structure):
    """The v-packet log consolidated on the device: CSR offsets + packet-ordered columns (tardis_mc_get_vpacket_log)."""
    _fields_ = (
        [("capacity", C.c_int64), ("count", C.c_int64), ("offsets", _pi), ("source_packet", _pi)]
        + [(n, _pd) for n in _VL_F64]
        + [(n, _pi) for n in _VL_I64]
    )


class TardisMcDecomposition(C.Structure):
    """The emitted spectrum decomposed by last interaction (tardis_mc_packet_decomposition): inputs, host output pointers, counts."""
    _fields_ = (
        [("n_classes", C.c_int64), ("line_class", _pi), ("time_of_simulation", C.c_double), ("nu_start", C.c_double),
         ("nu_end", C.c_double)]
        + [(n, _pd) for n in ("emission", "absorption", "no_interaction", "electron_scatter")]
        + [(n, _pi) for n in ("shell_packets", "line_emit_packets", "line_absorb_packets")]
        + [(n, C.c_int64) for n in ("n_selected", "n_line", "n_electron_scatter", "n_no_interaction")]
    )


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_pd)


def _ip(a: np.ndarray):
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(_pi)


class Marshalled:
    """A ctypes struct plus the numpy arrays that back its pointers (kept alive together)."""

    def __init__(self, struct, keep):
        self.struct = struct
        self.keep = keep

    def ref(self):
        return C.byref(self.struct)


def marshal_packets(pc) -> Marshalled:
    arrs = [np.ascontiguousarray(getattr(pc, n), dtype=np.float64)
            for n in ("initial_radii", "initial_nus", "initial_mus", "initial_energies")]
    seeds = np.ascontiguousarray(pc.packet_seeds, dtype=np.int64)
    n = len(arrs[0])
    if not all(len(a) == n for a in arrs) or len(seeds) != n:
        raise ValueError("packet arrays must have equal length")
    s = TardisMcPackets(n, _dp(arrs[0]), _dp(arrs[1]), _dp(arrs[2]), _dp(arrs[3]), _ip(seeds))
    return Marshalled(s, arrs + [seeds])


def marshal_geometry(geometry, time_explosion=None) -> Marshalled:
    r_in = np.ascontiguousarray(geometry.r_inner, dtype=np.float64)
    r_out = np.ascontiguousarray(geometry.r_outer, dtype=np.float64)
    t = float(geometry.time_explosion if time_explosion is None else time_explosion)
    if len(r_in) != len(r_out):
        raise ValueError("r_inner / r_outer length mismatch")
    return Marshalled(TardisMcGeometry(len(r_in), _dp(r_in), _dp(r_out), t), [r_in, r_out])


def marshal_opacity(op) -> Marshalled:
    ne = np.ascontiguousarray(op.electron_density, dtype=np.float64)
    nu = np.ascontiguousarray(op.line_list_nu, dtype=np.float64)
    tau = np.ascontiguousarray(op.tau_sobolev, dtype=np.float64)  # shell slices are strided views
    prob = np.ascontiguousarray(op.transition_probabilities, dtype=np.float64)
    l2m = np.ascontiguousarray(op.line2macro_level_upper, dtype=np.int64)
    edge = np.ascontiguousarray(op.macro_block_edge_index, dtype=np.int64)
    ttype = np.ascontiguousarray(op.transition_type, dtype=np.int64)
    dest = np.ascontiguousarray(op.destination_level_id, dtype=np.int64)
    tline = np.ascontiguousarray(op.transition_line_id, dtype=np.int64)
    L, S = tau.shape
    if len(nu) != L or len(ne) != S:
        raise ValueError("tau_sobolev must be [n_lines, n_shells]")
    if prob.ndim == 2 and prob.shape == (1, 1) and S > 1 and len(edge) <= 1 and len(ttype) <= 1:
        # line_interaction_type "scatter": OpacityState.to_numba passes np.zeros((1, 1)) and size-1 macro tables
        # (tardis/opacities/opacity_state.py:199-209); the engine wants one column per shell
        prob = np.zeros((1, S))
    T = prob.shape[0]
    if prob.ndim != 2 or prob.shape[1] != S:
        raise ValueError("transition_probabilities must be [n_transitions, n_shells]")
    s = TardisMcOpacity(L, S, T, len(edge), _dp(ne), _dp(nu), _dp(tau), _dp(prob), _ip(l2m), _ip(edge), _ip(ttype),
                        _ip(dest), _ip(tline))
    return Marshalled(s, [ne, nu, tau, prob, l2m, edge, ttype, dest, tline])


def marshal_line_data(ld, n_transitions) -> Marshalled:
    """ld: an object with f_lu, wavelength_cm, g_lower, g_upper, level_lower, level_upper, n_levels, sobolev_coefficient and
    transition_probability_coef (None in scatter mode), e.g. synthetic.LineData."""
    f = [np.ascontiguousarray(getattr(ld, n), dtype=np.float64) for n in ("f_lu", "wavelength_cm", "g_lower", "g_upper")]
    lv = [np.ascontiguousarray(getattr(ld, n), dtype=np.int64) for n in ("level_lower", "level_upper")]
    L = len(f[0])
    if not all(len(a) == L for a in f + lv):
        raise ValueError("line data arrays must have n_lines entries")
    coef = ld.transition_probability_coef
    keep = f + lv
    s = TardisMcLineData(L, int(n_transitions), int(ld.n_levels), _dp(f[0]), _dp(f[1]), _dp(f[2]), _dp(f[3]), _ip(lv[0]), _ip(lv[1]),
                         None, float(ld.sobolev_coefficient))
    if coef is not None:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if len(coef) != int(n_transitions):
            raise ValueError("transition_probability_coef must have n_transitions entries")
        s.transition_probability_coef = _dp(coef)
        keep.append(coef)
    return Marshalled(s, keep)


def marshal_opacity_update(level_number_density, n_shells, electron_density=None, j_blues_mode=J_BLUES_DILUTE_BLACKBODY, t_radiative=None,
                           dilution_factor=None, time_of_simulation=0.0, volume=None, w_epsilon=0.0,
                           detailed_optical_window=False) -> Marshalled:
    S = int(n_shells)
    n = np.ascontiguousarray(level_number_density, dtype=np.float64)
    if n.ndim != 2 or n.shape[1] != S:
        raise ValueError("level_number_density must be [n_levels, n_shells]")
    s = TardisMcOpacityUpdate()
    s.level_number_density = _dp(n)
    s.j_blues_mode = int(j_blues_mode)
    s.time_of_simulation = float(time_of_simulation)
    s.w_epsilon = float(w_epsilon)
    s.detailed_optical_window = int(bool(detailed_optical_window))
    keep = [n]
    for name, value in (("electron_density", electron_density), ("t_radiative", t_radiative), ("dilution_factor", dilution_factor),
                        ("volume", volume)):
        if value is None:
            continue
        a = np.ascontiguousarray(value, dtype=np.float64)
        if a.shape != (S,):
            raise ValueError(f"{name} must have n_shells entries")
        setattr(s, name, _dp(a))
        keep.append(a)
    return Marshalled(s, keep)


def marshal_mean_opacity(t_radiative, bin_size, n_shells, n_bins, want_expansion=False) -> Marshalled:
    """The request of tardis_mc_mean_opacity with freshly allocated outputs: ``.out`` is the dict of them.  ``t_radiative`` None is
    passed as a missing pointer (the library refuses it)."""
    S, B = int(n_shells), int(n_bins)
    s = TardisMcMeanOpacity()
    s.bin_size = int(bin_size)
    keep = []
    if t_radiative is not None:
        t = np.ascontiguousarray(t_radiative, dtype=np.float64)
        if t.shape != (S,):
            raise ValueError("t_radiative must have n_shells entries")
        s.t_radiative = _dp(t)
        keep.append(t)
    out = {n: np.empty(S) for n in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland")}
    out["bins_low"], out["delta_nu"] = np.empty(B), np.empty(B)
    if want_expansion:
        out["kappa_expansion"] = np.empty((B, S))
    for name, a in out.items():
        setattr(s, name, _dp(a))
    m = Marshalled(s, keep + list(out.values()))
    m.out = out
    return m


def marshal_plasma_data(pd) -> Marshalled:
    """pd: an object with the fields of TardisMcPlasmaData as arrays (level_energy, level_g, level_metastable [K]; ion_level_edge
    [I+1]; element_ion_edge [E+1]; ion_charge, ionization_energy [I]; zeta_temperatures [NT]; zeta [I, NT]; number_density [E, S])
    and the scalars chi_0 and link_t_rad_t_electron, e.g. synthetic.PlasmaData.  The counts are taken from the array shapes."""
    f = {n: np.ascontiguousarray(getattr(pd, n), dtype=np.float64)
         for n in ("level_energy", "level_g", "ion_charge", "ionization_energy", "zeta_temperatures", "zeta", "number_density")}
    meta = np.ascontiguousarray(pd.level_metastable, dtype=np.int32)
    ion_edge = np.ascontiguousarray(pd.ion_level_edge, dtype=np.int64)
    elem_edge = np.ascontiguousarray(pd.element_ion_edge, dtype=np.int64)
    K, I, E, NT = len(f["level_energy"]), len(ion_edge) - 1, len(elem_edge) - 1, len(f["zeta_temperatures"])
    if f["number_density"].ndim != 2 or f["number_density"].shape[0] != E:
        raise ValueError("number_density must be [n_elements, n_shells]")
    if f["zeta"].shape != (I, NT):
        raise ValueError("zeta must be [n_ions, n_zeta_temperatures]")
    if len(f["level_g"]) != K or len(meta) != K or len(f["ion_charge"]) != I or len(f["ionization_energy"]) != I:
        raise ValueError("level arrays must have n_levels entries, ion arrays n_ions")
    s = TardisMcPlasmaData(K, I, E, f["number_density"].shape[1], NT, _dp(f["level_energy"]), _dp(f["level_g"]),
                           meta.ctypes.data_as(C.POINTER(C.c_int32)), _ip(ion_edge), _ip(elem_edge), _dp(f["ion_charge"]),
                           _dp(f["ionization_energy"]), _dp(f["zeta_temperatures"]), _dp(f["zeta"]), _dp(f["number_density"]),
                           float(pd.chi_0), float(pd.link_t_rad_t_electron))
    return Marshalled(s, list(f.values()) + [meta, ion_edge, elem_edge])


def marshal_nlte_data(nd) -> Marshalled:
    """nd: an object with species_ion [NS], species_line_edge [NS+1], line_id, A_ul, B_ul, B_lu [NL] and the flags
    coronal_approximation and classical_nebular, e.g. synthetic.NlteData.  The counts are taken from the array shapes."""
    ion = np.ascontiguousarray(nd.species_ion, dtype=np.int64)
    edge = np.ascontiguousarray(nd.species_line_edge, dtype=np.int64)
    line_id = np.ascontiguousarray(nd.line_id, dtype=np.int64)
    coef = [np.ascontiguousarray(getattr(nd, n), dtype=np.float64) for n in ("A_ul", "B_ul", "B_lu")]
    NS, NL = len(ion), len(line_id)
    if len(edge) != NS + 1:
        raise ValueError("species_line_edge must have n_species + 1 entries")
    if not all(len(a) == NL for a in coef):
        raise ValueError("A_ul, B_ul and B_lu must have one entry per NLTE line")
    s = TardisMcNlteData(NS, _ip(ion), NL, _ip(edge), _ip(line_id), _dp(coef[0]), _dp(coef[1]), _dp(coef[2]),
                         int(bool(nd.coronal_approximation)), int(bool(nd.classical_nebular)))
    return Marshalled(s, [ion, edge, line_id] + coef)


def marshal_nlte_collision_data(cd) -> Marshalled:
    """cd: an object with collision_temperatures [NT], species_pair_edge [NS+1], level_lower, level_upper, delta_e, g_ratio [NP] and
    C_ul [NP, NT], e.g. synthetic.NlteCollisionData.  The counts are taken from the array shapes."""
    temps = np.ascontiguousarray(cd.collision_temperatures, dtype=np.float64)
    edge = np.ascontiguousarray(cd.species_pair_edge, dtype=np.int64)
    lv = [np.ascontiguousarray(getattr(cd, n), dtype=np.int64) for n in ("level_lower", "level_upper")]
    f = [np.ascontiguousarray(getattr(cd, n), dtype=np.float64) for n in ("delta_e", "g_ratio")]
    c = np.ascontiguousarray(cd.C_ul, dtype=np.float64)
    NS, NT, NP = len(edge) - 1, len(temps), len(lv[0])
    if temps.ndim != 1 or edge.ndim != 1 or NS < 0:
        raise ValueError("collision_temperatures and species_pair_edge must be vectors")
    if not all(a.shape == (NP,) for a in lv + f):
        raise ValueError("level_lower, level_upper, delta_e and g_ratio must have one entry per pair")
    if c.shape != (NP, NT):
        raise ValueError("C_ul must be [n_pairs, n_temperatures]")
    s = TardisMcNlteCollisionData(NS, NT, _dp(temps), NP, _ip(edge), _ip(lv[0]), _ip(lv[1]), _dp(f[0]), _dp(f[1]), _dp(c))
    return Marshalled(s, [temps, edge, c] + lv + f)


def marshal_ionization_options(helium_treatment=None, helium_element=None, delta_treatment=None, plasma_data=None) -> Marshalled:
    """helium_treatment: None or "recomb-nlte" (anything else: ValueError); helium_element: the element row that is helium, None for
    the row where ``plasma_data.atomic_number == 2`` (ValueError when there is none); delta_treatment: None for the
    RadiationFieldCorrection expression, else the number that replaces it.  helium_element is resolved only with a helium treatment."""
    if helium_treatment not in HELIUM_TREATMENTS:
        raise ValueError(f"helium_treatment must be None or 'recomb-nlte', not {helium_treatment!r}")
    helium = HELIUM_TREATMENTS[helium_treatment]
    element = 0
    if helium:
        if helium_element is None:
            rows = np.flatnonzero(np.asarray(getattr(plasma_data, "atomic_number", ()), dtype=np.int64) == 2)
            if len(rows) == 0:
                raise ValueError("helium_treatment needs an element with atomic_number 2 in the plasma data, or helium_element")
            element = int(rows[0])
        else:
            element = int(helium_element)
    s = TardisMcIonizationOptions(helium, int(delta_treatment is not None), element, 0.0 if delta_treatment is None else float(delta_treatment))
    return Marshalled(s, [])


def marshal_continuum_data(cd) -> Marshalled:
    """cd: an object with level [NC], block_edge [NC+1], nu and x_sect [NP], e.g. synthetic.ContinuumData.  The counts are taken from
    the array shapes; what the arrays must hold is the library's to check."""
    level = np.ascontiguousarray(cd.level, dtype=np.int64)
    edge = np.ascontiguousarray(cd.block_edge, dtype=np.int64)
    nu = np.ascontiguousarray(cd.nu, dtype=np.float64)
    x = np.ascontiguousarray(cd.x_sect, dtype=np.float64)
    if level.ndim != 1 or edge.shape != (len(level) + 1,):
        raise ValueError("block_edge must have n_continua + 1 entries")
    if nu.ndim != 1 or x.shape != nu.shape:
        raise ValueError("nu and x_sect must be vectors of one length")
    s = TardisMcContinuumData(len(level), _ip(level), _ip(edge), len(nu), _dp(nu), _dp(x))
    return Marshalled(s, [level, edge, nu, x])


def marshal_bf_estimator_setup(t_electrons, n_shells) -> Marshalled:
    t = np.ascontiguousarray(t_electrons, dtype=np.float64)
    if t.shape != (int(n_shells),):
        raise ValueError("t_electrons must be [n_shells]")
    return Marshalled(TardisMcBfEstimatorSetup(_dp(t)), [t])


def marshal_continuum_query(nu, shell, n_continua, each=False) -> Marshalled:
    """The request of tardis_mc_continuum_opacity for the pairs (nu[q], shell[q]); ``m.out`` holds the output arrays: chi_bf_tot,
    chi_ff, n_current [n] and, with ``each``, chi_bf_each and x_sect_each [n, n_continua]."""
    nu = np.ascontiguousarray(np.atleast_1d(nu), dtype=np.float64)
    shell = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(shell), nu.shape), dtype=np.int64)
    if nu.ndim != 1:
        raise ValueError("nu must be a vector")
    n = len(nu)
    out = {"chi_bf_tot": np.empty(n), "chi_ff": np.empty(n), "n_current": np.empty(n, dtype=np.int64)}
    if each:
        out["chi_bf_each"], out["x_sect_each"] = np.empty((n, int(n_continua))), np.empty((n, int(n_continua)))
    s = TardisMcContinuumQuery()
    s.n, s.nu, s.shell = n, _dp(nu), _ip(shell)
    for name, a in out.items():
        setattr(s, name, _ip(a) if a.dtype == np.int64 else _dp(a))
    m = Marshalled(s, [nu, shell] + list(out.values()))
    m.out = out
    return m


def marshal_kpacket_query(shell, z_process, z_nu, force_kind=None, force_continuum=None) -> Marshalled:
    """The request of tardis_mc_kpacket_sample for the k-packets (shell[q], z_process[q], z_nu[q]); ``shell`` may be one number for
    all.  ``force_kind`` (one number or [n]; -1 samples) sets the kind, and ``force_continuum`` (likewise; -1 where none is forced) the
    continuum of kinds 2 and 3.  ``m.out`` holds the output arrays: kind, continuum (int64) and nu [n]."""
    z_process = np.ascontiguousarray(np.atleast_1d(z_process), dtype=np.float64)
    if z_process.ndim != 1:
        raise ValueError("z_process must be a vector")
    z_nu = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(z_nu), z_process.shape), dtype=np.float64)
    shell = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(shell), z_process.shape), dtype=np.int64)
    n = len(z_process)
    out = {"kind": np.empty(n, dtype=np.int64), "continuum": np.empty(n, dtype=np.int64), "nu": np.empty(n)}
    keep = [shell, z_process, z_nu] + list(out.values())
    s = TardisMcKpacketQuery()
    s.n, s.shell, s.z_process, s.z_nu = n, _ip(shell), _dp(z_process), _dp(z_nu)
    s.kind, s.continuum, s.nu = _ip(out["kind"]), _ip(out["continuum"]), _dp(out["nu"])
    if force_kind is not None or force_continuum is not None:
        fk = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(-1 if force_kind is None else force_kind), z_process.shape), dtype=np.int64)
        fc = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(-1 if force_continuum is None else force_continuum), z_process.shape), dtype=np.int64)
        s.force_kind, s.force_continuum = _ip(fk), _ip(fc)
        keep += [fk, fc]
    m = Marshalled(s, keep)
    m.out = out
    return m


def marshal_plasma_update(t_radiative, dilution_factor, n_shells, ionization_mode=0, excitation_mode=0,
                          j_blues_mode=J_BLUES_DILUTE_BLACKBODY, time_of_simulation=0.0, volume=None, w_epsilon=0.0,
                          detailed_optical_window=False) -> Marshalled:
    S = int(n_shells)
    s = TardisMcPlasmaUpdate()
    s.ionization_mode, s.excitation_mode, s.j_blues_mode = int(ionization_mode), int(excitation_mode), int(j_blues_mode)
    s.time_of_simulation = float(time_of_simulation)
    s.w_epsilon = float(w_epsilon)
    s.detailed_optical_window = int(bool(detailed_optical_window))
    keep = []
    for name, value in (("t_radiative", t_radiative), ("dilution_factor", dilution_factor), ("volume", volume)):
        if value is None:
            continue
        a = np.ascontiguousarray(value, dtype=np.float64)
        if a.shape != (S,):
            raise ValueError(f"{name} must have n_shells entries")
        setattr(s, name, _dp(a))
        keep.append(a)
    return Marshalled(s, keep)


def marshal_config(cfg, spectrum_frequency_grid, number_of_vpackets=None, sigma_thomson=None) -> Marshalled:
    grid = np.ascontiguousarray(spectrum_frequency_grid, dtype=np.float64)
    if sigma_thomson is None:
        # modes/classic/solver.py:291-300: disable_electron_scattering -> sigma_T = 1e-200
        sigma_thomson = 1e-200 if getattr(cfg, "DISABLE_ELECTRON_SCATTERING", False) else st.SIGMA_THOMSON
    n_v = int(cfg.NUMBER_OF_VPACKETS if number_of_vpackets is None else number_of_vpackets)
    s = TardisMcConfig(
        int(bool(cfg.ENABLE_FULL_RELATIVITY)), int(cfg.LINE_INTERACTION_TYPE), int(bool(cfg.DISABLE_LINE_SCATTERING)),
        int(bool(cfg.ENABLE_VPACKET_TRACKING)), n_v, float(cfg.SURVIVAL_PROBABILITY), float(cfg.VPACKET_TAU_RUSSIAN),
        float(cfg.VPACKET_SPAWN_START_FREQUENCY), float(cfg.VPACKET_SPAWN_END_FREQUENCY), float(sigma_thomson),
        len(grid), _dp(grid))
    return Marshalled(s, [grid])


class ResultBuffers:
    """Owns (or borrows) the output arrays and exposes them through a TardisMcResult struct."""

    def __init__(self, n_packets, n_shells, n_lines, n_grid, output_nus=None, output_energies=None,
                 trackers: st.LastInteractionTrackers | None = None, vpacket_log_capacity=0,
                 want_line_estimators=True, want_packet_outputs=True):
        P, S, L = int(n_packets), int(n_shells), int(n_lines)
        if want_packet_outputs:
            self.output_nus = output_nus if output_nus is not None else np.full(P, -99.0)
            self.output_energies = output_energies if output_energies is not None else np.full(P, -99.0)
            for a in (self.output_nus, self.output_energies):
                if a.dtype != np.float64 or not a.flags.c_contiguous or len(a) != P:
                    raise ValueError("output arrays must be contiguous float64 of length n_packets")
        else:  # the per-packet results stay on the device (NULL pointers: the library skips those copies)
            self.output_nus = self.output_energies = None
        self.j_estimator = np.zeros(S)
        self.nu_bar_estimator = np.zeros(S)
        self.j_blue_estimator = np.zeros((L, S)) if want_line_estimators else None
        self.edotlu_estimator = np.zeros((L, S)) if want_line_estimators else None
        self.v_packets_energy_hist = np.zeros(int(n_grid))
        self.trackers = trackers
        cap = int(vpacket_log_capacity)
        self.vpacket_nus = np.empty(cap)
        self.vpacket_energies = np.empty(cap)
        self.vpacket_initial_mus = np.empty(cap)
        self.vpacket_initial_rs = np.empty(cap)
        r = TardisMcResult()
        if want_packet_outputs:
            r.output_nus = _dp(self.output_nus)
            r.output_energies = _dp(self.output_energies)
        r.j_estimator = _dp(self.j_estimator)
        r.nu_bar_estimator = _dp(self.nu_bar_estimator)
        if want_line_estimators:
            r.j_blue_estimator = _dp(self.j_blue_estimator)
            r.edotlu_estimator = _dp(self.edotlu_estimator)
        r.v_packets_energy_hist = _dp(self.v_packets_energy_hist)
        if trackers is not None:
            m = {"li_radius": "radius", "li_nu": "nu", "li_energy": "energy", "li_before_nu": "before_nu",
                 "li_before_mu": "before_mu", "li_before_energy": "before_energy", "li_after_nu": "after_nu",
                 "li_after_mu": "after_mu", "li_after_energy": "after_energy"}
            for k, v in m.items():
                setattr(r, k, _dp(getattr(trackers, v)))
            m = {"li_shell_id": "shell_id", "li_interaction_type": "interaction_type",
                 "li_line_absorb_id": "interaction_line_absorb_id", "li_line_emit_id": "interaction_line_emit_id",
                 "li_interactions_count": "interactions_count"}
            for k, v in m.items():
                setattr(r, k, _ip(getattr(trackers, v)))
        r.vpacket_log_capacity = cap
        if cap:
            r.vpacket_nus = _dp(self.vpacket_nus)
            r.vpacket_energies = _dp(self.vpacket_energies)
            r.vpacket_initial_mus = _dp(self.vpacket_initial_mus)
            r.vpacket_initial_rs = _dp(self.vpacket_initial_rs)
        r.first_error_packet = -1
        self.struct = r

    def ref(self):
        return C.byref(self.struct)

    @property
    def counters(self) -> dict:
        return dict(zip(COUNTER_NAMES, [int(v) for v in self.struct.counters]))

    @property
    def vpacket_log_count(self) -> int:
        return int(self.struct.vpacket_log_count)
