"""tardis_mc_source_function held element by element to the exact level solve of tests/source_function_exact.py, on hand-built tables with
planted estimators (tardis_mc_debug_set_line_estimators):

  (a) the level sums alone (downbranch), one table per group width of the level index and the one-level table: (n_k + 1) u e_k against the
      exact sum, exactly 0 without lines;
  (b) the iteration on acyclic tables of depth <= 12, one per group width of the incoming-row index: 16 iterations, every level within
      2 w B_k + 1e-14 C_k of the exact C_k, the three line arrays bit for bit from the device's own C;
  (c) the stop rule: a weak two-level block (scale 1e-6 with p = 0.99, 1e-8 with p = 0.999) at six positions of 300 levels, in one of
      five shells, beside strong blocks; and a well-mixed cyclic table;
  (d) the refusals: NaN and +inf in one estimator cell, the bound on the iterations;
  (e) the closing kernel's grid stride on 262 401 lines.

Every bound is derived in source_function_exact.py, none is measured.  Under the former stop rule (max|dC| <= 1e-14 max|C| per shell) the
cases of (c) with a weak block failed with |C_dev - C| of 1e5 .. 1e7 times the bound on the weak levels: see profiles/source_function_exact.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import source_function_exact as sfx  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        yield eng


def install(eng, case, j_blue=None, edotlu=None):
    eng.set_geometry(case.geometry, case.time_explosion)
    eng.set_opacity(case.op)
    eng.set_config(case.config, case.grid)
    eng.debug_set_line_estimators(case.j_blue if j_blue is None else j_blue, case.edotlu if edotlu is None else edotlu)


def check_lines_bitwise(case, out, wavelength_cm=None):
    want = sfx.close_bitwise(case, out["e_dot_u"], wavelength_cm)
    for key in ("att_S_ul", "Jred_lu", "Jblue_lu"):
        assert np.array_equal(out[key], want[key]), (case.name, key, int((out[key] != want[key]).sum()))


def check_levels(case, out, bound, want="C"):
    ratio, where = sfx.worst_ratio(case, out["e_dot_u"], bound, want)
    print(case.name, "| worst |C_dev - C| / bound", ratio, "at (shell, level)", where)
    assert ratio <= 1.0, (case.name, ratio, where)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [0] + list(sfx.SHAPES))
def test_row_sums(engine, G):
    case = sfx.row_sum_case(G)
    install(engine, case)
    out = engine.source_function(case.t_sim, case.volume)
    assert engine.last_source_iterations() == 0
    print(case.name, "| group width, long rows:", {k: (g, int(l.sum())) for k, (g, l) in case.widths().items()})
    check_levels(case, out, sfx.sum_bound(case), want="e")
    check_lines_bitwise(case, out)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", list(sfx.SHAPES))
def test_iteration_on_acyclic_tables(engine, G):
    case = sfx.acyclic_case(G)
    install(engine, case)
    out = engine.source_function(case.t_sim, case.volume)
    assert engine.last_source_iterations() == 16
    print(case.name, "| group width, long rows:", {k: (g, int(l.sum())) for k, (g, l) in case.widths().items()})
    check_levels(case, out, sfx.level_bound(case))
    check_lines_bitwise(case, out)
    wave = 1.0e-5 * (1.0 + np.arange(case.L) / case.L)
    out_w = engine.source_function(case.t_sim, case.volume, wavelength_cm=wave)
    assert np.array_equal(out_w["e_dot_u"], out["e_dot_u"])
    check_lines_bitwise(case, out_w, wave)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shell", sfx.STOP_SHELLS)
@pytest.mark.parametrize("position", sfx.STOP_POSITIONS)
@pytest.mark.parametrize("table", list(sfx.STOP_TABLES))
def test_stop_rule_with_a_weak_block(engine, table, position, shell):
    case = sfx.stop_rule_case(table, position, shell)
    engine.set_option("source_max_iterations", 400_000)
    try:
        install(engine, case)
        out = engine.source_function(case.t_sim, case.volume)
        its = engine.last_source_iterations()
        again = engine.source_function(case.t_sim, case.volume)
    finally:
        engine.set_option("source_max_iterations", 20_000)
    print(case.name, "| iterations", its)
    check_levels(case, out, sfx.level_bound(case))
    check_lines_bitwise(case, out)
    for key in out:
        assert np.array_equal(out[key], again[key]), key


def test_stop_rule_on_a_well_mixed_table(engine):
    case = sfx.mixed_case()
    install(engine, case)
    out = engine.source_function(case.t_sim, case.volume)
    its = engine.last_source_iterations()
    print(case.name, "| iterations", its)
    assert 16 < its < 20_000 and its % 16 == 0
    check_levels(case, out, sfx.level_bound(case))
    check_lines_bitwise(case, out)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(engine):
    case = sfx.mixed_case()
    nu = case.op.line_list_nu
    freqs = np.linspace(nu[-1] * 1.05, nu[0] * 0.95, 8)
    install(engine, case)
    good = engine.source_function(case.t_sim, case.volume)
    engine.formal_integral_resident(1.0e4, freqs, 50)
    for shell, value in ((1, np.nan), (2, np.inf)):
        ed = case.edotlu.copy()
        line = int(np.flatnonzero(case.op.tau_sobolev[:, shell] > 1e-3)[0])  # (a line whose term is not 0 times the estimator)
        ed[line, shell] = value
        engine.debug_set_line_estimators(case.j_blue, ed)
        with pytest.raises(RuntimeError, match=r"\(-7\).*NaN or infinite rates in shell %d " % shell):
            engine.source_function(case.t_sim, case.volume)
        with pytest.raises(RuntimeError, match=r"\(-7\)"):  # nothing resident is left valid
            engine.formal_integral_resident(1.0e4, freqs, 50)
        engine.debug_set_line_estimators(case.j_blue, case.edotlu)  # a call after a refusal works again
        after = engine.source_function(case.t_sim, case.volume)
        for key in good:
            assert np.array_equal(after[key], good[key]), key
        engine.formal_integral_resident(1.0e4, freqs, 50)
    engine.set_option("source_max_iterations", 32)
    try:
        with pytest.raises(RuntimeError, match=r"\(-7\).*not converged after 32 iterations.*worst shell"):
            engine.source_function(case.t_sim, case.volume)
        assert engine.last_source_iterations() == 32
        with pytest.raises(RuntimeError, match=r"\(-7\)"):
            engine.formal_integral_resident(1.0e4, freqs, 50)
    finally:
        engine.set_option("source_max_iterations", 20_000)
    after = engine.source_function(case.t_sim, case.volume)
    for key in good:
        assert np.array_equal(after[key], good[key]), key
    # planting drops the resident source function, as a reset does
    engine.debug_set_line_estimators(case.j_blue, case.edotlu)
    with pytest.raises(RuntimeError, match=r"\(-7\)"):
        engine.formal_integral_resident(1.0e4, freqs, 50)


def test_planted_estimators_come_back_and_need_opacity_and_config():
    from tardis_amd.engine import Engine
    case = sfx.row_sum_case(4)
    with Engine(0) as eng:
        eng.set_geometry(case.geometry, case.time_explosion)
        eng.set_opacity(case.op)
        with pytest.raises(RuntimeError, match=r"\(-7\)"):  # no configuration yet
            eng.debug_set_line_estimators(case.j_blue, case.edotlu)
        eng.set_option("estimator_copies", 4)
        eng.set_config(case.config, case.grid)
        eng.debug_set_line_estimators(case.j_blue, case.edotlu)
        res = eng.get_results(track_last_interaction=False, want_packet_outputs=False)
        assert np.array_equal(res.j_blue_estimator, case.j_blue) and np.array_equal(res.edotlu_estimator, case.edotlu)
        assert not res.j_estimator.any() and not res.nu_bar_estimator.any()
        out = eng.source_function(case.t_sim, case.volume)
        eng.debug_set_line_estimators(case.j_blue, case.edotlu)  # planted a second time: the copies a reduction folded in are zeroed again
        again = eng.source_function(case.t_sim, case.volume)
        for key in out:
            assert np.array_equal(out[key], again[key]), key
    with Engine(0) as one_copy:
        install(one_copy, case)
        ref = one_copy.source_function(case.t_sim, case.volume)
        for key in out:
            assert np.array_equal(out[key], ref[key]), key


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------

def test_closing_kernel_grid_stride(engine):
    case = sfx.stride_case()
    assert case.L == 262144 + 257 and case.S == 2
    install(engine, case)
    out = engine.source_function(case.t_sim, case.volume)
    assert engine.last_source_iterations() == 16
    assert (out["e_dot_u"][[0, 2, 3, 4]] > 0).all() and (out["e_dot_u"][1] > 0).all()  # (level 1 has no line: its rate comes from the jumps)
    check_lines_bitwise(case, out)
    assert np.count_nonzero(out["att_S_ul"]) > case.L
