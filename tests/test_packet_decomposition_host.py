"""The last-interaction decomposition without a GPU: the yardstick (tests/packet_decomposition_ref.py) on an oracle run, the host
implementation of tardis_amd.spectrum against it, the ABI pieces, and the accumulation-path rule as a pure function
(tardis_amd/csrc/decomposition_plan.hpp, compiled with the host C++ compiler as tests/test_propagate_plan.py does)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import packet_decomposition_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib, spectrum, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tardis_amd", "csrc")
S, L, P, B, C = 5, 3000, 4099, 37, 7


@pytest.fixture(scope="module")
def oracle_run(oracle):
    prob = synthetic.make_problem(seed=7, n_packets=P, n_shells=S, n_lines=L, n_bins=B, log_tau_mean=-2.0,
                                  line_interaction_type="macroatom", level_sizes="heavy")
    run = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE)
    assert run.return_code == 0
    return prob, run


def test_the_yardstick_conserves_the_emitted_spectrum(oracle_run):
    prob, run = oracle_run
    t, grid = prob.packet_collection.time_of_simulation, prob.spectrum_frequency_grid
    cls = np.arange(L) % C
    out, n = ref.decompose(run.output_nus, run.output_energies, t, grid, run.trackers, cls, C, S)
    assert out["n_selected"] == out["n_line"] + out["n_electron_scatter"] + out["n_no_interaction"]
    assert out["n_selected"] == int((run.output_energies >= 0).sum()) > 1000
    assert out["n_line"] > 1000 and out["n_electron_scatter"] > 50 and out["n_no_interaction"] > 100
    assert out["shell_packets"][:C].sum() == out["n_line"] and out["shell_packets"][C].sum() == out["n_electron_scatter"]
    assert out["line_emit_packets"].sum() == out["n_line"] == out["line_absorb_packets"].sum()
    assert (out["shell_packets"][:C].sum(axis=1) > 0).all() and (out["shell_packets"].sum(axis=0) > 0).all()  # every class, every shell
    # the three kinds add up to the emitted histogram: both sides sum the same non-negative addends of a bin in some order
    emitted = run.output_energies >= 0
    lum = run.output_energies[emitted] / t
    hist, _ = np.histogram(run.output_nus[emitted], grid, weights=lum)
    n_bin = np.histogram(run.output_nus[emitted], grid)[0]
    total = out["emission"].sum(axis=0) + out["no_interaction"] + out["electron_scatter"]
    assert n_bin.sum() < emitted.sum()  # some output frequencies are off the grid
    # (numpy's weighted histogram takes differences of a running sum over ALL packets: its error scales with the whole sum)
    assert np.all(np.abs(total - hist) <= emitted.sum() * ref.U * lum.sum())
    exact, _ = ref._cells(np.zeros(int(n_bin.sum()), dtype=np.int64), ref.bins_of(run.output_nus[emitted], grid)[1],
                          lum[ref.bins_of(run.output_nus[emitted], grid)[0]], (B,))
    assert ref.within_bound(total, exact, n_bin + 2)  # (the sum of three partial sums: two more roundings)
    assert np.array_equal(n["emission"].sum(axis=0) + n["no_interaction"] + n["electron_scatter"], n_bin)


@pytest.mark.parametrize("window", [(0.0, np.inf), (4.0e14, 1.5e15)])
def test_host_implementation_equals_the_yardstick(oracle_run, window):
    prob, run = oracle_run
    t, grid, trk = prob.packet_collection.time_of_simulation, prob.spectrum_frequency_grid, run.trackers
    cls = np.arange(L) % C
    want, n = ref.decompose(run.output_nus, run.output_energies, t, grid, trk, cls, C, S, *window)
    got = spectrum.packet_decomposition(run.output_nus, run.output_energies, t, grid, trk.interaction_type, trk.interaction_line_emit_id,
                                        trk.interaction_line_absorb_id, trk.before_nu, trk.shell_id, cls, S, None, *window)
    assert 0 < want["n_selected"] and (window[0] == 0.0 or want["n_selected"] < int((run.output_energies >= 0).sum()))
    ref.assert_matches(got, want, n, "host")
    with pytest.raises(ValueError):
        spectrum.packet_decomposition(run.output_nus, run.output_energies, t, grid, trk.interaction_type, trk.interaction_line_emit_id,
                                      trk.interaction_line_absorb_id, trk.before_nu, trk.shell_id, cls, S, C - 1)


def test_transport_state_uses_the_host_implementation_without_a_resident_run(oracle_run):
    from tardis_amd import transport
    prob, run = oracle_run
    pc = prob.packet_collection
    ts = transport.MonteCarloTransportState(pc, prob.geometry, prob.opacity_state, prob.time_explosion)
    pc.output_nus[:], pc.output_energies[:] = run.output_nus, run.output_energies
    ts.tracker_last_interaction = run.trackers
    cls = np.arange(L) % C
    want, n = ref.decompose(run.output_nus, run.output_energies, pc.time_of_simulation, prob.spectrum_frequency_grid, run.trackers, cls, C, S)
    ref.assert_matches(ts.packet_decomposition(prob.spectrum_frequency_grid, cls), want, n, "state")


def test_species_classes():
    z = np.array([26, 14, 26, 8, 14, 26])
    ion = np.array([1, 1, 2, 0, 1, 1])
    cls, labels = spectrum.species_classes(z, ion)
    assert labels.tolist() == [800, 1401, 2601, 2602]
    assert cls.tolist() == [2, 1, 3, 0, 1, 2] and cls.dtype == np.int64
    cls, labels = spectrum.species_classes(z)
    assert labels.tolist() == [8, 14, 26] and cls.tolist() == [2, 1, 2, 0, 1, 2]


def test_header_symbols_and_struct():
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    assert "int tardis_mc_packet_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d);" in header
    assert "#define TARDIS_MC_ABI_VERSION 2 " in header
    assert "tardis_mc_packet_decomposition" in _lib.SYMBOLS
    assert ctypes.sizeof(_abi.TardisMcDecomposition) == 16 * 8
    assert [f[0] for f in _abi.TardisMcDecomposition._fields_] == [
        "n_classes", "line_class", "time_of_simulation", "nu_start", "nu_end", "emission", "absorption", "no_interaction",
        "electron_scatter", "shell_packets", "line_emit_packets", "line_absorb_packets", "n_selected", "n_line", "n_electron_scatter",
        "n_no_interaction"]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(_lib.lib(), "tardis_mc_packet_decomposition")
    from tardis_amd.engine import Engine
    from tardis_amd.transport import MonteCarloTransportState
    assert callable(getattr(Engine, "packet_decomposition", None)) and callable(getattr(MonteCarloTransportState, "packet_decomposition", None))


SHIM = r"""
#include "decomposition_plan.hpp"
extern "C" int path_shim(long long c, long long b, long long s) { return decomp::choose_path(c, b, s); }
extern "C" long long bytes_shim(long long c, long long b, long long s) { return decomp::private_bytes(c, b, s); }
extern "C" long long budget_shim() { return decomp::LDS_BUDGET_BYTES; }
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to compile decomposition_plan.hpp")
    d = tmp_path_factory.mktemp("decomposition_plan")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.path_shim, lib.bytes_shim):
        f.argtypes = [ctypes.c_longlong] * 3
    lib.bytes_shim.restype = lib.budget_shim.restype = ctypes.c_longlong
    return lib


# the private copy of a workgroup: (2 C + 2) B doubles, (C + 1) S counts and the four scalar counts, 8 bytes each, against 64 KiB
PATHS = [
    ((7, 37, 5), "privatised"),       # the tests' base shape: 4 736 + 320 + 32 bytes
    ((1, 1, 1), "privatised"),
    ((7, 1, 1), "privatised"),
    ((40, 300, 5), "direct"),         # 196 800 bytes of cells
    ((30, 10000, 20), "direct"),      # SDEC
    ((1, 2000, 20), "privatised"),    # 64 000 + 320 + 32 = 64 352 <= 65 536
    ((1, 2037, 20), "privatised"),    # 65 184 + 320 + 32 = 65 536: exactly the budget
    ((1, 2038, 20), "direct"),        # 32 bytes over
    ((1, 2037, 21), "direct"),        # 16 bytes over
    ((3, 1000, 20), "privatised"),    # 64 000 + 640 + 32
    ((3, 1024, 20), "direct"),        # 65 536 + 640 + 32
    ((100, 10, 100), "direct"),       # the shell counts alone: 80 800
    ((2**31 - 1, 1, 1), "direct"),    # no overflow in the rule
    ((1, 2**40, 1), "direct"),
    ((1, 1, 2**40), "direct"),
]


@pytest.mark.parametrize("shape,want", PATHS)
def test_path_choice(plan, shape, want):
    c, b, s = shape
    assert ("privatised", "direct")[plan.path_shim(c, b, s)] == want
    nbytes = ((2 * c + 2) * b + (c + 1) * s + 4) * 8
    if max(shape) <= 8192:
        assert plan.bytes_shim(c, b, s) == nbytes
    assert (nbytes <= plan.budget_shim()) == (want == "privatised")


def test_two_workgroups_fit_a_compute_unit(plan):
    assert 2 * plan.budget_shim() <= 160 * 1024
