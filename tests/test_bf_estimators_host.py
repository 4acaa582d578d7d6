"""Photo-ionisation and heating estimators, what can be pinned without a GPU: the plan routes option bf_estimators as it routes
track_full on every input tests/test_propagate_plan.py enumerates; the messages of tardis_mc_check_bf_estimator_setup; the symbols
and the struct; and the reference (tests/bf_estimator_ref.py) against three records computed by hand, operation by operation."""
import ctypes
import math
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bf_estimator_ref as bref  # noqa: E402
import test_propagate_plan as tpp  # noqa: E402
from tardis_amd import _abi, _lib, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("tardis_mc_set_bf_estimators", "tardis_mc_check_bf_estimator_setup", "tardis_mc_get_bf_estimators", "tardis_mc_get_segment_log",
               "tardis_mc_debug_bf_accumulate", "tardis_mc_last_bf_estimator_ms", "tardis_mc_bf_estimator_rates", "tardis_mc_get_bf_estimator_rates")

# the shim of tests/test_propagate_plan.py with the new input as its last integer
SHIM = tpp.SHIM.replace("int pfx_negative,", "int pfx_negative, int bf_estimators,").replace(
    "in.pfx_negative = pfx_negative != 0;", "in.pfx_negative = pfx_negative != 0; in.bf_estimators = bf_estimators != 0;")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    assert "bf_estimators" in SHIM
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("bf_plan")
    src = d / "plan_shim.cpp"
    src.write_text(SHIM)
    so = d / "plan_shim.so"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", tpp.CSRC, "-o", str(so), str(src)], check=True)
    f = ctypes.CDLL(str(so)).plan_shim
    i, ll = ctypes.c_int, ctypes.c_longlong
    f.argtypes = [i, i, i, ll, ll, ctypes.c_double] + [i] * 8 + [ll] + [i] * 5 + [ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, i]
    f.restype = i
    return f


def plan(shim, d, bf):
    out = (ctypes.c_int * 6)()
    msg = ctypes.create_string_buffer(512)
    rc = shim(*[d[k] for k in tpp.FIELDS], int(bf), out, msg, 512)
    return rc, list(out), msg.value


@pytest.mark.parametrize("name,expect,parts,kw,gpu", tpp.ROWS, ids=[r[0] for r in tpp.ROWS])
def test_bf_estimators_routes_like_track_full(shim, name, expect, parts, kw, gpu):
    """Every input of the plan's own test: with bf_estimators on and track_full off the plan is the one of track_full on (and both on:
    the same again); with the option off it is the row's own."""
    d = tpp.inputs_of(parts, kw)
    tracked = plan(shim, dict(d, track_full=1), 0)
    assert plan(shim, dict(d, track_full=0), 1) == tracked
    assert plan(shim, dict(d, track_full=1), 1) == tracked
    rc, out, msg = plan(shim, d, 0)
    if expect[0] == "error":
        assert rc == tpp.INVALID and expect[1] in msg.decode()
    else:
        assert rc == 0 and (out[0], out[1], bool(out[2])) == expect


def test_the_instrumented_variants(shim):
    """Written from the rule: variant 2 where the wave-owner kernel can run the call, else the lane kernel."""
    d = tpp.inputs_of([], {})
    assert plan(shim, d, 1)[1][0] == 2 and plan(shim, dict(d, variant=0), 1)[1][0] == 0
    assert plan(shim, dict(d, variant=3), 1)[1][0] == 2 and plan(shim, dict(d, lines_sorted=0), 1)[1][0] == 0


def test_check_function_messages():
    assert Engine.check_bf_estimator_setup([5000.0, 9000.0, 1e-300]) == (0, "")
    for bad, index in (([5000.0, 0.0, 7000.0], 1), ([-1.0, 5000.0], 0), ([5000.0, 6000.0, np.nan], 2), ([np.inf], 0)):
        rc, msg = Engine.check_bf_estimator_setup(bad)
        assert rc == _abi.ERR_INVALID_ARGUMENT
        assert f"t_electrons[{index}]" in msg and "not finite and positive" in msg
    L = _lib.lib()
    assert L.tardis_mc_check_bf_estimator_setup(None, 3) == _abi.ERR_INVALID_ARGUMENT and b"pointer is missing" in L.tardis_mc_last_error(None)
    m = _abi.marshal_bf_estimator_setup([1.0], 1)
    assert L.tardis_mc_check_bf_estimator_setup(m.ref(), 0) == _abi.ERR_INVALID_ARGUMENT and b"n_shells" in L.tardis_mc_last_error(None)
    with pytest.raises(ValueError):
        _abi.marshal_bf_estimator_setup([1.0, 2.0], 3)


def test_symbols_struct_and_header():
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header
    assert ctypes.sizeof(_abi.TardisMcBfEstimatorSetup) == 8
    for text in ("update_bound_free_estimators", "THIS PROJECT'S DECISION: a move of length zero writes no record", '"segment_log_capacity"',
                 '"continuum_field"', "tardis_mc_allreduce_estimators does not carry the tables"):
        assert text in header
    for method in ("set_bf_estimators", "get_bf_estimators", "get_segment_log", "debug_bf_accumulate", "bf_estimator_rates", "last_bf_estimator_ms",
                   "check_bf_estimator_setup"):
        assert callable(getattr(Engine, method))


def test_covering_continuum_helper():
    prob = synthetic.make_problem(seed=3, n_packets=64, n_shells=4, n_lines=300)
    lo, hi = synthetic.comoving_frequency_range(prob)
    nus = np.concatenate((prob.packet_collection.initial_nus, prob.opacity_state.line_list_nu))
    assert 0 < lo < nus.min() and nus.max() < hi
    ld = synthetic.make_line_data(3, prob.opacity_state, n_levels=60, time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(3, ld, 4)
    cd = synthetic.make_covering_continuum_data(pd, [(np.array([lo, hi]), np.array([1.0, 2.0])), (np.linspace(lo, hi, 5), np.ones(5))])
    assert list(cd.block_edge) == [0, 2, 7] and np.all(np.diff(cd.level) > 0)
    assert Engine.check_continuum_data(cd, pd) == (0, "")
    with pytest.raises(ValueError):
        synthetic.make_covering_continuum_data(pd, [(np.array([2.0, 1.0]), np.ones(2))])


def test_reference_against_three_hand_computed_records():
    """One continuum of three points; records at nu_min (first interval, x_sect[first]), at nu_max and inside the second interval, in
    two shells.  Every operation below is written out on Python floats in the header's order."""
    h, k_b = 6.62606957e-27, 1.3806488e-16
    b = [1.0e15, 2.0e15, 4.0e15]
    x = [3.0 * 2.0 ** -60, 2.0 ** -60, 2.0 ** -62]  # (~2.6e-18 cm^2; dyadic, so that the interpolation at a grid point is exact)
    cd = SimpleNamespace(level=np.array([0]), block_edge=np.array([0, 3]), nu=np.array(b), x_sect=np.array(x))
    t_e = [9000.0, 6000.0]
    recs = [(1.0e15, 2.5e10, 0), (4.0e15, 1.5e10, 1), (3.0e15, 4.0e10, 1)]
    hand = {name: [0.0, 0.0] for name in bref.TABLES}
    per_shell = {name: [[], []] for name in bref.TABLES}
    x_seen = []
    for nu, ed, s in recs:
        if nu == b[0]:
            lo, hi = 0, 1      # searchsorted gives 0, clipped to 1
        elif nu == b[2]:
            lo, hi = 1, 2
        else:
            lo, hi = 1, 2      # 2e15 < 3e15 < 4e15
        interval, hw, lw = b[hi] - b[lo], nu - b[lo], b[hi] - nu
        x_c = ((x[hi] * hw) + (x[lo] * lw)) / interval
        x_seen.append(x_c)
        beta_e = 1 / (k_b * t_e[s])
        bfac = float(bref.exp(np.array([(h * nu) * (-beta_e)]))[0])
        inc = (ed * x_c) / nu
        heat = (ed * x_c) * (1.0 - b[0] / nu)
        for name, v in zip(bref.TABLES, (inc, inc * bfac, heat, heat * bfac)):
            per_shell[name][s].append(v)
    assert x_seen[0] == x[0] and x_seen[1] == x[2] and x_seen[2] == ((x[2] * 1.0e15) + (x[1] * 1.0e15)) / 2.0e15
    for name in bref.TABLES:
        hand[name] = [math.fsum(per_shell[name][0]), math.fsum(per_shell[name][1])]
    got = bref.tables(cd, t_e, 2, [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
    for name in bref.TABLES:
        assert got[name].tolist() == [hand[name]], name
    assert got["statistics"].tolist() == [[1, 2]]
    assert got["bf_heating"][0, 0] == 0.0 and got["photo_ion"][0, 0] == (2.5e10 * x[0]) / 1.0e15   # at the threshold: no heating
    # one ulp outside either end: not current
    out = bref.tables(cd, t_e, 2, [np.nextafter(1.0e15, 0.0), np.nextafter(4.0e15, np.inf)], [1.0, 1.0], [0, 0])
    assert not out["statistics"].any() and not out["photo_ion"].any()
    r = bref.rates(got, 3.0e5, [2.0e40, 5.0e40])
    assert r["gamma_est"][0, 1] == got["photo_ion"][0, 1] * (1.0 / ((3.0e5 * 5.0e40) * h))
