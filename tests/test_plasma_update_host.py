"""The device plasma update without a GPU: the ABI pieces, the partition-form rule (tardis_amd/csrc/plasma_update_plan.hpp through
tardis_mc_plasma_update_path), and the yardstick (tests/plasma_update_ref.py) against a plain Python-loop form of the specification and
against its own invariants, on a planted model that holds every edge of the arithmetic and on a synthetic one."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tardis_mc_set_plasma_data", "tardis_mc_update_plasma", "tardis_mc_get_plasma", "tardis_mc_plasma_update_path",
               "tardis_mc_last_plasma_update_ms")
MODES = [(i, e) for i in ("nebular", "lte") for e in ("dilute-lte", "lte")]
EPS = 2.0 ** -52


def synthetic_model(seed=7, n_shells=6, n_lines=600, n_levels=900, largest_ion=300):
    prob = synthetic.make_problem(seed=seed, n_packets=16, n_shells=n_shells, n_lines=n_lines, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(seed, prob.opacity_state, n_levels=n_levels, time_explosion=prob.time_explosion)
    return synthetic.make_plasma_data(seed, ld, n_shells, largest_ion=largest_ion), ld


@pytest.fixture(scope="module")
def planted(oracle):
    pd, ld, prob, t_rad, w, facts = ref.planted_model()
    return pd, ld, prob, t_rad, w, facts, ref.solve(pd, t_rad, w)


@pytest.fixture(scope="module")
def models(oracle, planted):
    pd_s, _ = synthetic_model()
    return {"planted": (planted[0], planted[3], planted[4]), "synthetic": (pd_s, pd_s.t_radiative, pd_s.dilution_factor)}


def test_symbols_in_the_library_the_loader_and_the_header():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, header)
    for struct, fields in (("TardisMcPlasmaData", _abi.TardisMcPlasmaData._fields_), ("TardisMcPlasmaUpdate", _abi.TardisMcPlasmaUpdate._fields_)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        declared = re.findall(r"(\w+);", body)
        assert declared == [f[0] for f in fields]  # same fields, same order
    # five int64, ten pointers, two doubles; two pointers, three int32 (+ padding), double, pointer, double, int32 (+ padding)
    assert inspect.isclass(_abi.TardisMcPlasmaData) and _abi.C.sizeof(_abi.TardisMcPlasmaData) == 17 * 8
    assert _abi.C.sizeof(_abi.TardisMcPlasmaUpdate) == 16 + 16 + 8 + 8 + 8 + 8
    for text in ("x sqrt(x)", "compensated", "1024 shells"):  # what the header has to say about pow, pandas and the single workgroup
        assert text in header


def test_engine_and_solver_methods_exist():
    sig = inspect.signature(Engine.update_plasma)
    assert list(sig.parameters)[:6] == ["self", "t_radiative", "dilution_factor", "ionization", "excitation", "j_blues_mode"]
    assert sig.parameters["ionization"].default == "nebular" and sig.parameters["excitation"].default == "dilute-lte"
    assert list(inspect.signature(Engine.set_plasma_data).parameters) == ["self", "plasma_data"]
    assert list(inspect.signature(Engine.get_plasma).parameters) == ["self", "level_number_density", "ion_number_density", "partition_function",
                                                                     "electron_density"]
    sig = inspect.signature(transport.MCTransportSolverHIP.update_plasma)
    assert list(sig.parameters)[:6] == ["self", "t_radiative", "dilution_factor", "ionization", "excitation", "radiative_rates_type"]
    assert hasattr(transport.MCTransportSolverHIP, "set_plasma_data")
    solver = transport.MCTransportSolverHIP(synthetic.make_spectrum_grid(10), resident=False)
    with pytest.raises(RuntimeError, match="resident"):
        solver.update_plasma(np.ones(3), np.ones(3))
    assert list(inspect.signature(synthetic.make_plasma_data).parameters)[:3] == ["seed", "line_data", "n_shells"]


def test_partition_form_rule_on_both_sides_of_its_threshold():
    path = _lib.lib().tardis_mc_plasma_update_path
    threshold = int(re.search(r"LONG_BLOCK_ROWS = (\d+);", open(os.path.join(ROOT, "tardis_amd", "csrc", "opacity_update_plan.hpp")).read()).group(1))
    src = open(os.path.join(ROOT, "tardis_amd", "csrc", "plasma_update_plan.hpp")).read()
    assert "LONG_ION_LEVELS = opup::LONG_BLOCK_ROWS;" in src and "#include <hip" not in src  # the opacity update's rule; host only
    assert [path(n) for n in (0, 1, threshold - 1)] == [0, 0, 0]
    assert [path(n) for n in (threshold, threshold + 1, 900, 1 << 40)] == [1, 1, 1, 1]
    assert path(-5) == 0
    assert Engine.plasma_update_path(threshold - 1) == "lane" and Engine.plasma_update_path(threshold) == "row"
    assert _lib.lib().tardis_mc_opacity_update_path(threshold) == 1 and _lib.lib().tardis_mc_opacity_update_path(threshold - 1) == 0


def test_marshalling_takes_the_counts_from_the_arrays(planted):
    pd, *_ = planted
    m = _abi.marshal_plasma_data(pd)
    s = m.struct
    assert (s.n_levels, s.n_ions, s.n_elements, s.n_shells, s.n_zeta_temperatures) == (300, 12, 3, 4, 20)
    assert s.chi_0 == synthetic.CHI_0_CA_II and s.link_t_rad_t_electron == 0.9
    assert [s.ion_level_edge[i] for i in (0, 1, 12)] == [0, 12, 300] and s.level_metastable[0] == 1 and s.zeta[19] == pd.zeta[0, 19]
    u = _abi.marshal_plasma_update(pd.t_radiative, pd.dilution_factor, 4, 1, 0)
    assert (u.struct.ionization_mode, u.struct.excitation_mode, u.struct.j_blues_mode) == (1, 0, 0) and not bool(u.struct.volume)
    assert u.struct.t_radiative[3] == 40000.0
    with pytest.raises(ValueError):
        _abi.marshal_plasma_update(pd.t_radiative, pd.dilution_factor, 5)
    import copy
    bad = copy.copy(pd)
    bad.zeta = pd.zeta[:, :-1]
    with pytest.raises(ValueError):
        _abi.marshal_plasma_data(bad)


def _loops(pd, t_rad, w, ionization, excitation, exp):
    """The specification, one shell and one cell at a time; the all-shells vote at the end of every pass."""
    K, I, E, S = len(pd.level_g), len(pd.ion_charge), len(pd.element_ion_edge) - 1, len(t_rad)
    k_b, h, m_e = ref.K_BOLTZMANN, ref.H_PLANCK, ref.M_ELECTRON
    ie, ee = [int(v) for v in pd.ion_level_edge], [int(v) for v in pd.element_ion_edge]
    zt = [float(v) for v in pd.zeta_temperatures]
    lbf, z, phi = np.zeros((K, S)), np.zeros((I, S)), np.full((I, S), np.nan)
    n_e = [0.0] * S
    for s in range(S):
        t, ws = float(t_rad[s]), float(w[s])
        beta_rad = 1 / (k_b * t)
        t_e = pd.link_t_rad_t_electron * t
        beta_e = 1 / (k_b * t_e)
        x = ((2 * np.pi * m_e) / beta_rad) / (h * h)
        g_e = x * float(np.sqrt(x))
        for i in range(I):
            acc = 0.0
            for k in range(ie[i], ie[i + 1]):
                v = float(pd.level_g[k]) * exp(float(pd.level_energy[k]) * (-beta_rad))
                if excitation == "dilute-lte" and not pd.level_metastable[k]:
                    v = v * ws
                lbf[k, s] = v
                acc = acc + v
            z[i, s] = acc
        hi = 0
        while hi < len(zt) and zt[hi] < t:
            hi += 1
        hi = min(max(hi, 1), len(zt) - 1)
        lo = hi - 1
        for e in range(E):
            for i in range(ee[e], ee[e + 1] - 1):
                chi = float(pd.ionization_energy[i])
                p = (z[i + 1, s] / z[i, s]) * ((2 * g_e) * exp(chi * (-beta_rad)))
                if ionization == "nebular":
                    slope = (float(pd.zeta[i, hi]) - float(pd.zeta[i, lo])) / (zt[hi] - zt[lo])
                    zeta = slope * (t - zt[lo]) + float(pd.zeta[i, lo])
                    fa = t_e / (((1 / ws) * ws) * t)
                    if chi >= pd.chi_0:
                        delta = fa * exp(chi * (beta_rad - beta_e))
                    else:
                        delta = (1 - exp(chi * beta_rad - beta_rad * pd.chi_0)) + fa * exp(chi * beta_rad - beta_e * pd.chi_0)
                    p = ((p * ws) * ((zeta * delta) + ws * (1 - zeta))) * float(np.sqrt(t_e / t))
                phi[i, s] = p
            n_e[s] = n_e[s] + float(pd.number_density[e, s])
    n_ion, passes = np.zeros((I, S)), 0
    while True:
        done = True
        for s in range(S):
            new = 0.0
            for e in range(E):
                cps, total, cp = [], 0.0, 1.0
                for i in range(ee[e], ee[e + 1] - 1):
                    pe = float(np.nan_to_num(np.float64(phi[i, s]) / np.float64(n_e[s])))
                    cp = pe if i == ee[e] else cp * pe
                    cps.append(cp)
                    total = total + cp
                n0 = float(pd.number_density[e, s]) / (1 + total)
                for j, i in enumerate(range(ee[e], ee[e + 1])):
                    n = n0 if j == 0 else n0 * cps[j - 1]
                    if n < 1e-20:
                        n = 0.0
                    n_ion[i, s] = n
                    new = new + n * float(pd.ion_charge[i])
            if not abs(new - n_e[s]) / n_e[s] < 0.05:
                done = False
            n_e[s] = (new, n_e[s])
        passes += 1
        if done:
            n_e = [old for _, old in n_e]
            break
        n_e = [0.5 * (new + old) for new, old in n_e]
    ion = ref.level_ion(pd)
    n = np.array([[(lbf[k, s] / z[ion[k], s]) * n_ion[ion[k], s] for s in range(S)] for k in range(K)])
    return {"level_number_density": n, "ion_number_density": n_ion, "partition_function": z, "electron_density": np.array(n_e), "iterations": passes}


@pytest.mark.parametrize("ionization,excitation", MODES)
def test_the_yardstick_equals_the_specification_cell_by_cell(planted, oracle, ionization, excitation):
    pd, ld, prob, t_rad, w, facts, _ = planted
    got = ref.solve(pd, t_rad, w, ionization, excitation)
    want = _loops(pd, t_rad, w, ionization, excitation, lambda x: float(oracle.exp_array(np.array([x]), 1)[0]))
    assert got["iterations"] == want["iterations"]
    for name in ("partition_function", "ion_number_density", "electron_density", "level_number_density"):
        assert np.array_equal(got[name], want[name]), name


def test_every_planted_case_is_present(planted):
    pd, ld, prob, t_rad, w, facts, out = planted
    levels = np.diff(pd.ion_level_edge)
    assert all(levels[i] == 1 for i in facts["one_level_ions"]) and levels[facts["long_ion"]] >= 40
    assert {Engine.plasma_update_path(int(n)) for n in levels} == {"lane", "row"}  # both forms of the partition kernel
    chi = pd.ionization_energy[levels > 1]
    assert (chi < pd.chi_0).any() and (chi > pd.chi_0).any() and (chi == pd.chi_0).any()  # both branches of delta, and the bound itself
    zt = pd.zeta_temperatures
    assert t_rad[facts["zeta_end_shells"][0]] == zt[0] and t_rad[facts["zeta_end_shells"][1]] == zt[-1] and t_rad[facts["zeta_node_shell"]] in zt[1:-1]
    assert not np.isin(t_rad[2], zt)
    lbf = out["level_boltzmann_factor"]
    assert lbf[facts["underflow_level"], facts["underflow_shell"]] == 0.0 and np.count_nonzero(lbf == 0.0) <= 4
    n_ion, n = out["ion_number_density"], out["level_number_density"]
    assert (n_ion == 0.0).sum() >= 4 and (n_ion[n_ion > 0] >= 1e-20).all() and ((n_ion > 0) & (n_ion < 1e-10)).any()
    assert (n[ld.level_lower] == 0.0).sum() > 100  # n_l == 0 cells for the opacity stages downstream
    per_shell = ref.passes_per_shell(out["deltas"])
    assert len(set(per_shell.tolist())) >= 3 and out["iterations"] == per_shell.max() == per_shell[facts["cold_thin_shell"]] >= 5
    assert min(np.abs(d - ref.THRESHOLD).min() for d in out["deltas"]) > 1e-9
    with pytest.raises(ref.PlasmaIonizationError):
        ref.solve(pd, t_rad, w, max_iterations=2)


@pytest.mark.parametrize("ionization,excitation", MODES)
@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_yardsticks_own_invariants(models, name, ionization, excitation):
    pd, t_rad, w = models[name]
    out = ref.solve(pd, t_rad, w, ionization, excitation)
    n_ion, n, n_e = out["ion_number_density"], out["level_number_density"], out["electron_density"]
    ee, ie = pd.element_ion_edge, pd.ion_level_edge
    # the ions of an element hold its atoms
    for e in range(len(ee) - 1):
        np.testing.assert_allclose(n_ion[ee[e]:ee[e + 1]].sum(axis=0), pd.number_density[e], rtol=1e-13, atol=0)
    # the levels of an ion hold its atoms: 4 ulp per level (lbf / Z and the product round once each; Z itself is the sum of the lbf, the
    # re-summation adds one rounding per level)
    for i in range(len(ie) - 1):
        levels = ie[i + 1] - ie[i]
        total = np.add.accumulate(n[ie[i]:ie[i + 1]], axis=0)[-1]
        assert np.all(np.abs(total - n_ion[i]) <= 4 * levels * np.spacing(n_ion[i])), (i, total, n_ion[i])
    # the electron density handed out is the one the last pass used, and it passes the 5 % test
    new = ref.serial_sum(ref.ion_populations(pd, out["phi"], n_e) * pd.ion_charge[:, None])
    assert np.all(np.abs(new - n_e) / n_e < ref.THRESHOLD) and out["iterations"] >= 2
    assert np.array_equal(ref.ion_populations(pd, out["phi"], n_e), n_ion)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_lte_with_unit_dilution_is_boltzmann_inside_an_ion(models, name):
    pd, t_rad, _ = models[name]
    out = ref.solve(pd, t_rad, np.ones(len(t_rad)), "lte", "lte")
    n, ie = out["level_number_density"], pd.ion_level_edge
    ge = pd.level_g[:, None] * ref.exp(pd.level_energy[:, None] * (-(1 / (ref.K_BOLTZMANN * t_rad)))[None, :])
    assert np.array_equal(out["level_boltzmann_factor"], ge)
    checked = 0
    for i in range(len(ie) - 1):
        a, b = ie[i], ie[i + 1]
        ok = (n[a:b] > 1e-290) & (n[a] > 1e-290)[None, :]  # (ratios of normal numbers only)
        with np.errstate(divide="ignore", invalid="ignore"):
            got, want = n[a:b] / n[a], ge[a:b] / ge[a]
        # each population is the Boltzmann factor rounded twice more (/ Z, * N), the ratios round once each: 6 roundings
        assert np.all(np.abs(got - want)[ok] <= 6 * EPS * want[ok]), i
        checked += int(ok.sum())
    assert checked > 500
    # and the dilute form is the same with W on the non-metastable levels
    dil = ref.solve(pd, t_rad, np.full(len(t_rad), 0.5), "lte", "dilute-lte")["level_boltzmann_factor"]
    meta = pd.level_metastable != 0
    assert np.array_equal(dil[meta], ge[meta]) and np.array_equal(dil[~meta], ge[~meta] * 0.5)


def test_partition_functions_agree_with_a_pandas_group_sum(models):
    pandas = pytest.importorskip("pandas")
    for pd, t_rad, w in models.values():
        lbf = ref.boltzmann_factors(pd, t_rad, w, "dilute-lte")
        z = ref.partition_functions(pd, lbf)
        grouped = pandas.DataFrame(lbf).groupby(ref.level_ion(pd)).sum().values
        np.testing.assert_allclose(z, grouped, rtol=1e-14, atol=0)  # (pandas compensates its sum: to rounding, not bitwise)


def test_synthetic_plasma_data_has_the_shape_it_promises():
    pd, ld = synthetic_model()
    levels = np.diff(pd.ion_level_edge)
    assert levels.sum() == ld.n_levels == len(pd.level_energy) and levels.min() == 1 and levels.max() == 300
    assert np.all(levels[np.asarray(pd.element_ion_edge[1:]) - 1] == 1)  # an element's last ion: one level
    assert np.median(levels) < levels.mean() / 2  # heavy-tailed
    assert np.all(np.diff(pd.element_ion_edge) == 5) and np.array_equal(pd.ion_charge[:5], np.arange(5.0))
    assert np.all(pd.level_energy[pd.ion_level_edge[:-1]] == 0.0) and np.all(pd.level_metastable[pd.ion_level_edge[:-1]] == 1)
    assert 0 < pd.level_metastable.mean() < 0.5 and np.all(pd.level_g >= 1)
    assert np.all(np.diff(pd.number_density, axis=1) < 0) and np.all((pd.zeta > 0) & (pd.zeta <= 1)) and (pd.zeta == 1.0).all(axis=1).any()
    chi = pd.ionization_energy[levels > 1]
    assert np.all((chi > 5 * synthetic.EV) & (chi < 200 * synthetic.EV)) and (chi < pd.chi_0).any() and (chi > pd.chi_0).any()
    assert pd.number_density.shape == (6, 6) and pd.zeta.shape == (30, 20)
