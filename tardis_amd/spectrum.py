"""Real-packet spectrum (the parity metric of BASELINE.json).

Restates SpectrumSolver.montecarlo_emitted_luminosity (tardis/spectrum/base.py:140-159) on plain arrays:
``np.histogram(emitted_packet_nu, weights=emitted_packet_luminosity, bins=spectrum_frequency_grid)`` with
emitted = output_energies >= 0 and luminosity = energy / time_of_simulation
(montecarlo_transport_state.py:130-160).
"""
from __future__ import annotations

import numpy as np


def emitted_luminosity_histogram(output_nus, output_energies, time_of_simulation, spectrum_frequency_grid):
    mask = output_energies >= 0
    lum = output_energies[mask] / time_of_simulation
    hist, _ = np.histogram(output_nus[mask], weights=lum, bins=spectrum_frequency_grid)
    return hist


def relative_l2(a, b) -> float:
    """||a - b||_2 / ||b||_2 (0 when both vanish)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = float(np.sqrt(np.sum(b * b)))
    num = float(np.sqrt(np.sum((a - b) ** 2)))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def reabsorbed_luminosity_histogram(output_nus, output_energies, time_of_simulation, spectrum_frequency_grid):
    """SpectrumSolver.montecarlo_reabsorbed_luminosity (tardis/spectrum/base.py:140-148)."""
    mask = output_energies < 0
    lum = -(output_energies[mask] / time_of_simulation)
    hist, _ = np.histogram(output_nus[mask], weights=lum, bins=spectrum_frequency_grid)
    return hist


def species_classes(atomic_number, ion_number=None):
    """The grouping of lines that SDEC uses, as ``(line_class, labels)``: ``labels`` the sorted unique species ids
    ``atomic_number * 100 + ion_number`` (``atomic_number`` alone with ``ion_number=None``: by element) and ``line_class[i]`` the
    index of line i's id in ``labels`` -- what ``packet_decomposition`` takes, with ``n_classes = len(labels)``."""
    ids = np.asarray(atomic_number, dtype=np.int64)
    if ion_number is not None:
        ids = ids * 100 + np.asarray(ion_number, dtype=np.int64)
    labels, line_class = np.unique(ids, return_inverse=True)
    return line_class.astype(np.int64).reshape(ids.shape), labels


def _weighted_histogram(x, w, grid):
    """numpy.histogram's bin assignment (left-closed bins, the last one closed on the right, nothing outside the grid) with one
    np.add.at per addend instead of its cumulative-sum differences: every bin is a plain sum of its own non-negative addends."""
    B = len(grid) - 1
    out = np.zeros(B)
    inside = (x >= grid[0]) & (x <= grid[-1])
    k = np.minimum(np.searchsorted(grid, x[inside], side="right") - 1, B - 1)
    np.add.at(out, k, w[inside])
    return out, inside, k


def packet_decomposition(output_nus, output_energies, time_of_simulation, spectrum_frequency_grid, interaction_type, line_emit_id,
                         line_absorb_id, before_nu, shell_id, line_class, n_shells, n_classes=None, nu_start=0.0, nu_end=np.inf):
    """The emitted spectrum decomposed by last interaction on the host, with the definitions of ``tardis_mc_packet_decomposition``
    (include/tardis_mc.h) and the same dict as ``Engine.packet_decomposition``: emission / absorption luminosity per line class and
    spectrum bin (SDEC), the no-interaction and electron-scattering spectra, packets per (emit class | electron scattering, shell)
    (LIV) and per emitting / absorbing line (LastLineInteraction), from the last-interaction tracker's arrays."""
    grid = np.asarray(spectrum_frequency_grid, dtype=np.float64)
    nu, en = np.asarray(output_nus, dtype=np.float64), np.asarray(output_energies, dtype=np.float64)
    cls = np.asarray(line_class, dtype=np.int64)
    L, S, B = len(cls), int(n_shells), len(grid) - 1
    C = int(n_classes) if n_classes is not None else (int(cls.max()) + 1 if L else 1)
    if C < 1 or (L and (cls.min() < 0 or cls.max() >= C)):
        raise ValueError("line_class values must be in [0, n_classes)")
    if not time_of_simulation > 0:
        raise ValueError("time_of_simulation must be positive")
    sel = (en >= 0) & (nu > nu_start) & (nu < nu_end)
    lum = en / time_of_simulation
    itype = np.asarray(interaction_type)
    line, es, none = sel & (itype == 2), sel & (itype == 4), sel & (itype == -1)
    emit, absorb = np.asarray(line_emit_id)[line], np.asarray(line_absorb_id)[line]
    out = {"emission": np.zeros((C, B)), "absorption": np.zeros((C, B)),
           "shell_packets": np.zeros((C + 1, S), dtype=np.int64)}
    for key, ids, x in (("emission", emit, nu[line]), ("absorption", absorb, np.asarray(before_nu, dtype=np.float64)[line])):
        _, inside, k = _weighted_histogram(x, lum[line], grid)
        np.add.at(out[key], (cls[ids[inside]], k), lum[line][inside])
    out["no_interaction"] = _weighted_histogram(nu[none], lum[none], grid)[0]
    out["electron_scatter"] = _weighted_histogram(nu[es], lum[es], grid)[0]
    shell = np.asarray(shell_id)
    np.add.at(out["shell_packets"], (cls[emit], shell[line]), 1)
    np.add.at(out["shell_packets"], (np.full(int(es.sum()), C), shell[es]), 1)
    out["line_emit_packets"] = np.bincount(emit, minlength=L).astype(np.int64)
    out["line_absorb_packets"] = np.bincount(absorb, minlength=L).astype(np.int64)
    out.update(n_selected=int(sel.sum()), n_line=int(line.sum()), n_electron_scatter=int(es.sum()), n_no_interaction=int(none.sum()))
    return out


def vpacket_decomposition(vpacket_nus, vpacket_energies, time_of_simulation, spectrum_frequency_grid, last_interaction_type,
                          last_interaction_out_id, last_interaction_in_id, last_interaction_in_nu, last_interaction_shell_id, line_class,
                          n_shells, n_classes=None, nu_start=0.0, nu_end=np.inf):
    """The VIRTUAL spectrum decomposed by last interaction on the host (SDEC / LIV with ``packets_mode="virtual"``), with the
    definitions of ``tardis_mc_vpacket_decomposition`` and the dict of ``Engine.vpacket_decomposition``: ``packet_decomposition`` on the
    columns of a v-packet log with last-interaction columns -- one entry per v-packet, its frequency and energy as outputs (never
    negative; a v-packet the roulette dropped adds 0.0 and still counts), the emitting line ``out_id``, the absorbing line ``in_id``."""
    return packet_decomposition(vpacket_nus, vpacket_energies, time_of_simulation, spectrum_frequency_grid, last_interaction_type,
                                last_interaction_out_id, last_interaction_in_id, last_interaction_in_nu, last_interaction_shell_id,
                                line_class, n_shells, n_classes, nu_start, nu_end)


def calculate_filtered_luminosity(packet_nu, packet_luminosity, luminosity_nu_start=0.0, luminosity_nu_end=np.inf):
    """tardis/spectrum/luminosity.py:5-30 on plain arrays."""
    f = (packet_nu > luminosity_nu_start) & (packet_nu < luminosity_nu_end)
    return packet_luminosity[f].sum()
