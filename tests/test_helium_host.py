"""helium_treatment recomb-nlte and delta_treatment of the device plasma step without a GPU: the yardstick (tests/helium_ref.py) against
tests/plasma_update_ref.py and against the facts of its planted model, the host-side check of the options
(tardis_mc_check_ionization_options through ctypes), the ABI struct and its marshaller, and synthetic.make_helium_plasma_data."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helium_ref as href  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tardis_mc_set_ionization_options", "tardis_mc_check_ionization_options", "tardis_mc_get_helium", "tardis_mc_last_helium_ms")
FIELDS = ("level_number_density", "ion_number_density", "partition_function", "phi", "electron_density", "level_boltzmann_factor")


@pytest.fixture(scope="module")
def planted(oracle):
    pd, ld, prob, t_rad, w, facts = href.planted_helium_model()
    arms = {"plain": ref.solve(pd, t_rad, w),
            "helium": href.solve(pd, t_rad, w, helium_element=2),
            "helium_delta": href.solve(pd, t_rad, w, helium_element=2, delta_treatment=1.0),
            "delta": href.solve(pd, t_rad, w, delta_treatment=0.3)}
    return pd, t_rad, w, facts, arms


def nearest(sol):
    return float(np.abs(np.stack(sol["deltas"]) - ref.THRESHOLD).min())


def test_the_planted_model_is_the_one_the_header_of_the_reference_describes(planted):
    pd = planted[0]
    assert pd.number_density.shape == (3, 4) and len(pd.level_energy) == 300
    assert list(np.diff(pd.ion_level_edge)[9:12]) == [20, 14, 1] and pd.atomic_number[2] == 2
    assert pd.ionization_energy[9] == 24.587 * href.EV and pd.ionization_energy[10] == 54.418 * href.EV
    for i in (9, 10):
        a, b = pd.ion_level_edge[i], pd.ion_level_edge[i + 1]
        excited = pd.level_energy[a + 1:b] / pd.ionization_energy[i]
        assert pd.level_energy[a] == 0.0 and excited.min() >= 0.78 and excited.max() <= 0.98 and np.all(np.diff(excited) >= 0)


def test_with_neither_option_the_restatement_is_the_plain_one(planted):
    pd, t_rad, w, _, arms = planted
    for ionization in ("nebular", "lte"):
        for excitation in ("dilute-lte", "lte"):
            want = arms["plain"] if (ionization, excitation) == ("nebular", "dilute-lte") else ref.solve(pd, t_rad, w, ionization, excitation)
            got = href.solve(pd, t_rad, w, ionization=ionization, excitation=excitation)
            assert got["iterations"] == want["iterations"] and got["helium_relative"] is None and got["helium_population"] is None
            for name in FIELDS:
                assert np.array_equal(got[name], want[name], equal_nan=True), name
            assert all(np.array_equal(a, b) for a, b in zip(got["deltas"], want["deltas"]))


def test_pass_counts_and_distance_to_the_threshold(planted):
    arms = planted[4]
    assert arms["helium"]["iterations"] == 6 and list(ref.passes_per_shell(arms["helium"]["deltas"])) == [6, 4, 5, 5]
    assert arms["helium_delta"]["iterations"] == 6 and arms["delta"]["iterations"] == 7
    # far from the 5 % threshold on the scale of an ulp: the pass count does not hang on a last bit
    assert 2.0e-3 < nearest(arms["helium"]) < 2.2e-3
    assert 1.0e-3 < nearest(arms["helium_delta"]) < 1.1e-3
    assert 2.1e-3 < nearest(arms["delta"]) < 2.3e-3


def test_facts_of_the_helium_arm(planted):
    pd, t_rad, w, facts, arms = planted
    sol, plain = arms["helium"], arms["plain"]
    a = facts["helium_ions"][0]
    k0, k3 = int(pd.ion_level_edge[a]), int(pd.ion_level_edge[a + 3])
    for arm in ("helium", "helium_delta", "delta"):
        for name in ("level_number_density", "ion_number_density", "electron_density"):
            assert np.isfinite(arms[arm][name]).all(), (arm, name)
    assert np.all(sol["level_number_density"][k0] == 0.0) and np.all(sol["helium_relative"][0] == 0.0)   # He I ground
    assert np.all(sol["helium_relative"][20] == 1.0)                                                       # He II ground
    assert np.array_equal(sol["level_number_density"][k0:k3], sol["helium_population"])
    total = sol["ion_number_density"][a:a + 3].sum(axis=0)
    assert np.all(np.abs(total - pd.number_density[2]) <= 2 * np.spacing(pd.number_density[2]))
    assert np.all(sol["electron_density"] != plain["electron_density"])
    # the plant that catches a 1e-20 cut applied to the helium rows: He III of the cold thin shell
    he3 = sol["ion_number_density"][a + 2, 0]
    assert 2.7e-131 < he3 < 2.9e-131
    # the other elements' rows are the ordinary chain's with this arm's n_e, the partition functions untouched
    assert np.array_equal(sol["partition_function"], plain["partition_function"])
    other = ref.ion_populations(pd, sol["phi"], sol["electron_density"])
    assert np.array_equal(sol["ion_number_density"][:a], other[:a]) and not np.array_equal(sol["ion_number_density"][a:a + 3], other[a:a + 3])
    ion = ref.level_ion(pd)
    n = (sol["level_boltzmann_factor"] / sol["partition_function"][ion]) * sol["ion_number_density"][ion]
    assert np.array_equal(sol["level_number_density"][:k0], n[:k0])


def test_delta_treatment_changes_phi_only_where_there_is_a_delta(planted):
    pd, t_rad, w, _, arms = planted
    assert not np.array_equal(arms["delta"]["phi"], arms["plain"]["phi"], equal_nan=True)
    assert np.array_equal(arms["delta"]["partition_function"], arms["plain"]["partition_function"])
    lte = href.solve(pd, t_rad, w, delta_treatment=0.3, ionization="lte")
    want = ref.solve(pd, t_rad, w, "lte")
    assert np.array_equal(lte["level_number_density"], want["level_number_density"]) and lte["iterations"] == want["iterations"]
    with pytest.raises(ValueError):
        href.solve(pd, t_rad, w, helium_element=2, ionization="lte")
    assert np.all(href.delta_values(pd, t_rad, w, 0.3) == 0.3)


def test_symbols_struct_and_header():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, header)
    body = re.search(r"typedef struct TardisMcIonizationOptions \{(.*?)\} TardisMcIonizationOptions;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in _abi.TardisMcIonizationOptions._fields_]
    assert C.sizeof(_abi.TardisMcIonizationOptions) == 4 + 4 + 8 + 8
    assert L.tardis_mc_abi_version() == 2 == _abi.ABI_VERSION
    for text in ("recomb-nlte", "NOT applied", "hp[k]", "numerical-nlte"):
        assert text in header
    for name in ("set_ionization_options", "get_helium", "last_helium_ms"):
        assert callable(getattr(Engine, name))
    assert callable(transport.MCTransportSolverHIP.set_ionization_options)


def test_the_marshaller(planted):
    pd = planted[0]
    m = _abi.marshal_ionization_options("recomb-nlte", None, None, pd)
    assert (m.struct.helium_treatment, m.struct.use_delta_treatment, m.struct.helium_element) == (1, 0, 2)   # resolved from atomic_number
    m = _abi.marshal_ionization_options("recomb-nlte", 1, 0.25, pd)
    assert (m.struct.helium_treatment, m.struct.use_delta_treatment, m.struct.helium_element, m.struct.delta_treatment) == (1, 1, 1, 0.25)
    m = _abi.marshal_ionization_options(None, None, 1.0)
    assert (m.struct.helium_treatment, m.struct.use_delta_treatment, m.struct.delta_treatment) == (0, 1, 1.0)
    no_helium = copy.copy(pd)
    no_helium.atomic_number = np.array([20, 26, 8])
    with pytest.raises(ValueError):
        _abi.marshal_ionization_options("recomb-nlte", None, None, no_helium)
    with pytest.raises(ValueError):
        _abi.marshal_ionization_options("numerical-nlte", None, None, pd)
    assert href.helium_element_of(pd) == 2
    with pytest.raises(ValueError):
        href.helium_element_of(no_helium)


def check(options, pd, **changes):
    """(return code, message) of tardis_mc_check_ionization_options on the tables of ``pd`` with ``changes``."""
    L = _lib.lib()
    t = {name: np.ascontiguousarray(changes.get(name, getattr(pd, name)), dtype=dtype)
         for name, dtype in (("element_ion_edge", np.int64), ("ion_level_edge", np.int64), ("ion_charge", np.float64))}
    rc = L.tardis_mc_check_ionization_options(C.byref(options), len(t["element_ion_edge"]) - 1, t["element_ion_edge"].ctypes.data,
                                              t["ion_level_edge"].ctypes.data, t["ion_charge"].ctypes.data)
    return rc, L.tardis_mc_last_error(None).decode()


def test_the_host_check_of_the_options(planted):
    pd = planted[0]
    opt = _abi.TardisMcIonizationOptions
    assert check(opt(1, 0, 2, 0.0), pd)[0] == 0
    assert check(opt(1, 1, 2, 1.0), pd)[0] == 0
    assert check(opt(0, 1, 0, 0.3), pd)[0] == 0
    assert check(opt(0, 0, -7, np.nan), pd)[0] == 0       # what is not switched on is not read
    E = len(pd.element_ion_edge) - 1
    four = pd.element_ion_edge.copy()                      # the helium element takes an ion of its neighbour: four ions
    four[2] -= 1
    charges = pd.ion_charge.copy()
    charges[11] = 3.0
    two_levels = pd.ion_level_edge.copy()                  # He III takes a level of He II
    two_levels[11] -= 1
    cases = ((opt(1, 0, -1, 0.0), {}, "helium_element -1"),
             (opt(1, 0, E, 0.0), {}, "helium_element %d" % E),
             (opt(1, 0, 2, 0.0), dict(element_ion_edge=four), "4 ions"),
             (opt(1, 0, 2, 0.0), dict(ion_charge=charges), "charges 0, 1, 3"),
             (opt(1, 0, 2, 0.0), dict(ion_level_edge=two_levels), "2 levels"),
             (opt(0, 1, 0, np.nan), {}, "delta_treatment is not finite"),
             (opt(1, 1, 2, np.inf), {}, "delta_treatment is not finite"),
             (opt(2, 0, 2, 0.0), {}, "unknown helium_treatment 2"))
    for options, changes, words in cases:
        rc, message = check(options, pd, **changes)
        assert rc == _abi.ERR_INVALID_ARGUMENT and words in message, (words, rc, message)
    L = _lib.lib()
    assert L.tardis_mc_check_ionization_options(None, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert L.tardis_mc_check_ionization_options(C.byref(opt(1, 0, 0, 0.0)), 3, None, None, None) == _abi.ERR_INVALID_ARGUMENT


def test_synthetic_helium_plasma_data_and_the_unchanged_plain_one():
    prob = synthetic.make_problem(seed=7, n_packets=16, n_shells=6, n_lines=600, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(7, prob.opacity_state, n_levels=900, time_explosion=prob.time_explosion)
    pd = synthetic.make_helium_plasma_data(7, ld, 6, helium_levels=(19, 10), largest_ion=300)
    assert pd.atomic_number[0] == 2 and list(pd.element_ion_edge[:2]) == [0, 3] and list(pd.ion_charge[:3]) == [0.0, 1.0, 2.0]
    assert list(np.diff(pd.ion_level_edge)[:3]) == [19, 10, 1] and pd.ion_level_edge[-1] == 900 == len(pd.level_energy)
    ev = synthetic.EV
    assert pd.ionization_energy[0] == 24.587387 * ev and pd.ionization_energy[1] == 54.417763 * ev
    assert list(pd.level_metastable[:3]) == [1, 1, 1] and 2 <= pd.level_metastable[1:19].sum() <= 3
    for i in (0, 1):
        a, b = pd.ion_level_edge[i], pd.ion_level_edge[i + 1]
        excited = pd.level_energy[a + 1:b] / pd.ionization_energy[i]
        assert excited.min() >= 0.78 and excited.max() <= 0.98 and np.all(np.diff(excited) >= 0)
    _abi.marshal_plasma_data(pd)
    assert _abi.marshal_ionization_options("recomb-nlte", None, None, pd).struct.helium_element == 0
    # the other elements are dealt as make_plasma_data deals them on the remaining levels
    rest = synthetic.make_plasma_data(7, copy.copy(ld).__class__(**{**ld.__dict__, "n_levels": 870}), 6, largest_ion=300)
    assert np.array_equal(pd.level_energy[30:], rest.level_energy) and np.array_equal(pd.zeta[3:], rest.zeta)
    assert np.array_equal(pd.ion_level_edge[3:], rest.ion_level_edge + 30) and np.array_equal(pd.atomic_number[1:], rest.atomic_number)
    assert np.allclose(pd.number_density.sum(axis=0), rest.number_density.sum(axis=0), rtol=1e-14)
