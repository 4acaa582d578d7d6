"""The collisional rates of the NLTE excitation stage without a GPU: the ABI pieces, what tardis_mc_set_nlte_collision_data refuses
(its host-side check through tardis_mc_check_nlte_collision_data) with the bounds rule of the temperature grid, the marshalling, and
the yardstick (tests/nlte_collision_ref.py) against scipy's interp1d, against numpy.linalg.solve and against the conditions the inputs
of tests/test_nlte_collision_gpu.py have to meet."""
import copy
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlte_collision_ref as cref  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
from tardis_amd import _abi, _lib, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tardis_mc_set_nlte_collision_data", "tardis_mc_check_nlte_collision_data", "tardis_mc_get_nlte_collision_rates")

# The largest relative difference of a population between the restatement and numpy.linalg.solve over the systems WITH collisional
# rates below (the four models, three shells, a first update on beta of ones and the resident n_e of set_opacity, a second on the
# first's beta_sobolev and solved n_e): the figure this run measures is asserted to be the one written here and in include/tardis_mc.h.
# The bound is the project's 1e-11 (tests/test_nlte_excitation_host.py) and the measurement must lie ten times below it.
LAPACK_MEASURED, LAPACK_BOUND = 1.7e-14, 1e-11


@pytest.fixture(scope="module")
def cases(oracle):
    """Per model of cref.test_models: the model, j, and the two updates' (beta, previous n_e, solution)."""
    out = cref.test_models()
    for m in out.values():
        nu = np.asarray(m["prob"].opacity_state.line_list_nu, dtype=np.float64)
        m["j"] = oref.j_blues_dilute_blackbody(nu, m["t_rad"], m["w"])
        args = (m["pd"], m["ld"], m["nd"], m["cd"], m["t_rad"], m["w"], m["j"])
        first = cref.solve(*args, None, m["n_e0"])
        beta = oref.update(m["ld"], m["prob"].opacity_state, m["prob"].time_explosion, first["level_number_density"], j_blues=m["j"])["beta_sobolev"]
        second = cref.solve(*args, beta, first["electron_density"])
        m["updates"] = ((None, m["n_e0"], first), (beta, first["electron_density"], second))
    return out


def test_symbols_in_the_library_the_loader_and_the_header():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, header)
    body = re.search(r"typedef struct TardisMcNlteCollisionData \{(.*?)\} TardisMcNlteCollisionData;", header, re.S).group(1)
    fields = [f[0] for f in _abi.TardisMcNlteCollisionData._fields_]
    assert re.findall(r"(\w+);", body) == fields  # same fields, same order
    assert fields == ["n_species", "n_temperatures", "collision_temperatures", "n_pairs", "species_pair_edge", "level_lower", "level_upper", "delta_e",
                      "g_ratio", "C_ul"]
    assert _abi.C.sizeof(_abi.TardisMcNlteCollisionData) == 10 * 8 and _abi.C.sizeof(_abi.TardisMcNlteData) == 72  # (the NLTE struct is not touched)
    for text in ("previous_electron_densities", "inv_g_ratio", "interp1d", "mcm::exp", "AT ENTRY", "%.2g" % LAPACK_MEASURED):
        assert text in header, text


def test_engine_solver_and_generator_signatures():
    assert list(inspect.signature(Engine.set_nlte_collision_data).parameters) == ["self", "collision_data"]
    assert list(inspect.signature(Engine.get_nlte_collision_rates).parameters) == ["self", "c_ul", "c_lu"]
    assert hasattr(transport.MCTransportSolverHIP, "set_nlte_collision_data")
    assert "collision" not in " ".join(inspect.signature(transport.MCTransportSolverHIP.update_plasma).parameters)  # a property of the data
    names = list(inspect.signature(synthetic.make_nlte_collision_data).parameters)
    assert names[:3] == ["seed", "plasma_data", "nlte_data"]
    assert {"pair_fraction", "n_temperatures", "nan_fraction", "magnitude", "reach_levels"} <= set(names)


def _levels(pd, nd):
    return np.ascontiguousarray(np.diff(pd.ion_level_edge)[np.asarray(nd.species_ion, dtype=np.int64)], dtype=np.int64)


def _check(cd, pd, nd, t_rad=None, n_species=None):
    m = _abi.marshal_nlte_collision_data(cd)
    levels = _levels(pd, nd)
    t = None if t_rad is None else np.ascontiguousarray(t_rad, dtype=np.float64)
    rc = _lib.lib().tardis_mc_check_nlte_collision_data(m.ref(), len(levels) if n_species is None else n_species, levels.ctypes.data,
                                                        float(pd.link_t_rad_t_electron), 0 if t is None else len(t), None if t is None else t.ctypes.data)
    return rc, _lib.lib().tardis_mc_last_error(None).decode()


def test_what_the_host_side_check_refuses(cases):
    c = cases["four"]
    pd, nd, good = c["pd"], c["nd"], c["cd"]
    assert _check(good, pd, nd)[0] == 0
    p70 = int(good.species_pair_edge[1])  # the first pair of the species of 70 levels
    p17 = int(good.species_pair_edge[3])  # ... and of 17

    def bad(text, n_species=None, **changes):
        cd = copy.copy(good)
        for k, v in changes.items():
            setattr(cd, k, v)
        rc, msg = _check(cd, pd, nd, n_species=n_species)
        assert rc == _abi.ERR_INVALID_ARGUMENT and text in msg, (rc, msg)

    def changed(name, index, value):
        a = getattr(good, name).copy()
        a[index] = value
        return {name: a}

    bad("the NLTE data have 5", n_species=5)                                    # a wrong n_species
    bad("the NLTE data have 4", species_pair_edge=good.species_pair_edge[:-1])
    bad("from 0 to", **changed("species_pair_edge", -1, len(good.level_lower) - 1))  # an edge table that does not run from 0 to NP
    bad("from 0 to", **changed("species_pair_edge", 0, 1))
    edge = good.species_pair_edge.copy()
    edge[1], edge[2] = edge[2], edge[1]
    bad("decreases", species_pair_edge=edge)
    bad("not both inside", **changed("level_upper", p70 + 3, 70))                # a level outside the species' ion
    bad("not both inside", **changed("level_lower", p70 + 3, -1))
    bad("not both inside", **changed("level_upper", p17, 17))                    # (inside the 70, outside the 17)
    bad("lower >= upper", **changed("level_lower", p70 + 3, good.level_upper[p70 + 3]))  # l >= u
    lower, upper = good.level_lower.copy(), good.level_upper.copy()
    lower[p70 + 3], upper[p70 + 3] = upper[p70 + 3], lower[p70 + 3]
    bad("lower >= upper", level_lower=lower, level_upper=upper)
    lower, upper = good.level_lower.copy(), good.level_upper.copy()
    lower[p70 + 4], upper[p70 + 4] = lower[p70 + 3], upper[p70 + 3]
    bad("repeated", level_lower=lower, level_upper=upper)                        # a repeated pair
    for value in (0.0, -1.0, np.inf, np.nan):
        bad("g_ratio", **changed("g_ratio", p70 + 3, value))                     # g_ratio not finite and positive
    for value in (np.inf, -np.inf, np.nan):
        bad("delta_e", **changed("delta_e", p70 + 3, value))                     # delta_e not finite
    bad("ascend", **changed("collision_temperatures", 3, good.collision_temperatures[2]))  # temperatures that do not ascend
    bad("ascend", **changed("collision_temperatures", 3, np.nan))
    bad("n_temperatures >= 2", collision_temperatures=good.collision_temperatures[:1], C_ul=good.C_ul[:, :1])  # NT < 2
    # a missing pointer: the struct by hand
    m = _abi.marshal_nlte_collision_data(good)
    levels = _levels(pd, nd)
    for field in ("collision_temperatures", "species_pair_edge", "level_lower", "level_upper", "delta_e", "g_ratio", "C_ul"):
        s = _abi.TardisMcNlteCollisionData.from_buffer_copy(m.struct)
        setattr(s, field, None)
        rc = _lib.lib().tardis_mc_check_nlte_collision_data(_abi.C.byref(s), 4, levels.ctypes.data, 0.9, 0, None)
        assert rc == _abi.ERR_INVALID_ARGUMENT and "pointer" in _lib.lib().tardis_mc_last_error(None).decode(), field
    assert _lib.lib().tardis_mc_check_nlte_collision_data(None, 4, levels.ctypes.data, 0.9, 0, None) == _abi.ERR_INVALID_ARGUMENT
    assert _lib.lib().tardis_mc_check_nlte_collision_data(m.ref(), 4, None, 0.9, 0, None) == _abi.ERR_INVALID_ARGUMENT
    # NaN in C_ul is data, and a species may have no pairs
    assert np.isnan(good.C_ul).any() and good.species_pair_edge[0] == good.species_pair_edge[1]
    with pytest.raises(ValueError):
        _abi.marshal_nlte_collision_data(dataclasses.replace(good, delta_e=good.delta_e[:-1]))
    with pytest.raises(ValueError):
        _abi.marshal_nlte_collision_data(dataclasses.replace(good, C_ul=good.C_ul[:, :-1]))


def test_marshalling_takes_the_counts_from_the_arrays(cases):
    cd = cases["four"]["cd"]
    s = _abi.marshal_nlte_collision_data(cd).struct
    assert (s.n_species, s.n_temperatures, s.n_pairs) == (4, 12, 2415 + int(np.diff(cd.species_pair_edge)[3]))
    assert [s.species_pair_edge[i] for i in range(5)] == list(cd.species_pair_edge)
    q = 2000
    assert (s.level_lower[q], s.level_upper[q], s.delta_e[q], s.g_ratio[q]) == (cd.level_lower[q], cd.level_upper[q], cd.delta_e[q], cd.g_ratio[q])
    assert s.C_ul[q * 12 + 5] == cd.C_ul[q, 5] and s.collision_temperatures[11] == cd.collision_temperatures[11]  # [NP][NT]


def test_the_bounds_rule_of_the_temperature_grid(cases):
    c = cases["four"]
    pd, nd, cd = c["pd"], c["nd"], c["cd"]
    link = pd.link_t_rad_t_electron
    first, last = cd.collision_temperatures[0], cd.collision_temperatures[-1]
    inside = np.array([9000.0, 10000.0, 11000.0])

    def t_rad_of(t_e):
        """A t_rad whose product with link is exactly t_e."""
        t = t_e / link
        for cand in (t, np.nextafter(t, 0), np.nextafter(t, np.inf)):
            if link * cand == t_e:
                return cand
        raise AssertionError(t_e)

    def rule(t_rad):
        rc, msg = _check(cd, pd, nd, t_rad)
        try:
            cref.collision_rates(cd, cref.electron_temperatures(pd, t_rad))
            ok = True
        except cref.CollisionBoundsError:
            ok = False
        assert (rc == 0) == ok and rc in (0, _abi.ERR_INVALID_ARGUMENT), (rc, msg)  # the library and the restatement agree
        return rc, msg

    assert rule(inside)[0] == 0
    for knot in (first, last):  # exactly on the first and on the last knot: accepted
        t = inside.copy()
        t[1] = t_rad_of(knot)
        assert link * t[1] == knot and rule(t)[0] == 0
    t = inside.copy()
    t[2] = np.nextafter(t_rad_of(first), 0)
    assert link * t[2] < first
    rc, msg = rule(t)
    assert rc == _abi.ERR_INVALID_ARGUMENT and "shell 2" in msg and "outside the collision temperatures" in msg
    t = inside.copy()
    t[0] = np.nextafter(t_rad_of(last), np.inf)
    assert link * t[0] > last
    rc, msg = rule(t)
    assert rc == _abi.ERR_INVALID_ARGUMENT and "shell 0" in msg
    t = inside.copy()
    t[1] = np.nan
    assert rule(t)[0] == _abi.ERR_INVALID_ARGUMENT


def test_the_interpolation_is_scipys(cases):
    """Which one was used: scipy.interpolate.interp1d (scipy is importable where this suite was written); np.interp, per pair, only
    where it is not.  Equal to 1e-15 relative on every finite value, NaN where the reference has NaN."""
    try:
        from scipy.interpolate import interp1d
        used = "scipy.interpolate.interp1d"
    except ImportError:
        interp1d, used = None, "np.interp"
    print("the interpolation is compared with", used)
    for name in ("four", "edges"):
        c = cases[name]
        cd = c["cd"]
        t_e = cref.electron_temperatures(c["pd"], c["t_rad"])
        got = cref.interpolate(cd.collision_temperatures, cd.C_ul, t_e)
        if interp1d is not None:
            want = interp1d(cd.collision_temperatures, cd.C_ul)(t_e)  # (as get_collision_matrix calls it: linear, bounds_error)
        else:
            want = np.stack([np.interp(t_e, cd.collision_temperatures, row) for row in cd.C_ul])
        finite = np.isfinite(want)
        assert finite.sum() > 0.6 * want.size and np.all(np.isnan(got[~finite]))
        assert np.max(np.abs(got[finite] - want[finite]) / np.abs(want[finite])) <= 1e-15
    edges = cases["edges"]
    t_e = cref.electron_temperatures(edges["pd"], edges["t_rad"])
    x = edges["cd"].collision_temperatures
    assert x[0] < t_e[0] < x[1] and t_e[1] in x[2:-2] and x[-2] < t_e[2] < x[-1]  # the first interval | a knot | the last interval
    c_ul = edges["updates"][0][2]["c_ul"]
    holes = np.isnan(edges["cd"].C_ul[:, 1])  # NaN at the upper knot of the first interval
    assert holes.sum() > 50 and np.all(c_ul[holes, 0] == 0.0) and np.all(c_ul[~np.isnan(edges["cd"].C_ul[:, 0]), 0] > 0) and np.all(c_ul[:, 1:] > 0)


def test_the_restatement_agrees_with_lapack(cases):
    worst, cond, count = {}, {}, 0
    for name, c in cases.items():
        worst[name], cond[name] = 0.0, 0.0
        for beta, n_e, _ in c["updates"]:
            for pos, s, k0, n, m in cref.species_systems(c["pd"], c["ld"], c["nd"], c["cd"], c["t_rad"], c["j"], beta, n_e):
                if c["cd"].species_pair_edge[pos] == c["cd"].species_pair_edge[pos + 1]:
                    continue  # (no collisional rates in this system: tests/test_nlte_excitation_host.py)
                b = np.zeros(n)
                b[0] = 1.0
                x, _ = nref.lu_solve(m, b)
                want = np.linalg.solve(m, b)
                worst[name] = max(worst[name], float(np.max(np.abs(x - want) / np.abs(want))))
                cond[name] = max(cond[name], float(np.linalg.cond(m)))
                count += 1
        print(f"restatement vs numpy.linalg.solve with collisional rates, model {name!r}: largest relative difference of a population "
              f"{worst[name]:.3g}, largest condition number {cond[name]:.3g}")
    worst = max(worst.values())
    assert count == 2 * 3 * (2 + 2 + 2 + 2)
    assert LAPACK_MEASURED / 2 <= worst <= LAPACK_MEASURED * 2  # the figure written above and in the header is the one this run measures
    assert worst <= LAPACK_BOUND / 10  # at least ten times below the bound: conditioning is a property of the inputs
    assert worst <= 1e-11


def _lbf(c, update, **terms):
    """{(position, shell): x / x[0]} of one update's systems, None where the solve fails."""
    beta, n_e, _ = update
    out = {}
    for pos, s, k0, n, m in cref.species_systems(c["pd"], c["ld"], c["nd"], c["cd"], c["t_rad"], c["j"], beta, n_e, **terms):
        b = np.zeros(n)
        b[0] = 1.0
        try:
            x = nref.lu_solve(m, b)[0]
            out[(pos, s)] = x / x[0]
        except nref.NlteSolveError:
            out[(pos, s)] = None
    return out


def test_neither_term_is_drowned(cases):
    """In every model of the GPU tests, and in both of its updates, there is a (species, shell) where dropping the collisional term
    changes some lbf by more than 1e-3 relative, and one where dropping the radiative term does (or makes the system singular)."""
    for name, c in cases.items():
        for update in c["updates"]:
            full, no_c, no_r = _lbf(c, update), _lbf(c, update, collisional=False), _lbf(c, update, radiative=False)

            def moved(other):
                return max(np.inf if other[k] is None else float(np.max(np.abs(other[k] - full[k]) / np.abs(full[k]))) for k in full if full[k] is not None)

            assert all(v is not None for v in full.values())
            assert moved(no_c) > 1e-3 and moved(no_r) > 1e-3, (name, moved(no_c), moved(no_r))
            finite = [float(np.max(np.abs(no_r[k] - full[k]) / np.abs(full[k]))) for k in full if no_r[k] is not None and len(full[k]) > 1]
            assert finite and max(finite) > 1e-3, name  # (not only through a singular system)


def test_the_inputs_have_the_shape_they_promise(cases):
    four, reached, boundary = cases["four"], cases["reached"], cases["boundary"]
    assert list(np.diff(four["cd"].species_pair_edge)[:3]) == [0, 70 * 69 // 2, 0] and 20 < np.diff(four["cd"].species_pair_edge)[3] < 17 * 16 // 2
    assert list(np.diff(boundary["cd"].species_pair_edge)) == [142 * 141 // 2, 141 * 140 // 2]
    for c in cases.values():
        cd = c["cd"]
        assert np.all(cd.level_lower < cd.level_upper) and np.all(cd.delta_e > 0) and np.all(np.diff(cd.collision_temperatures) > 0)
        for pos in range(len(cd.species_pair_edge) - 1):  # sorted by (lower, upper) within a species, hence unique
            a, b = cd.species_pair_edge[pos], cd.species_pair_edge[pos + 1]
            key = cd.level_lower[a:b] * 1000 + cd.level_upper[a:b]
            assert np.all(np.diff(key) > 0)
        nan = np.isnan(cd.C_ul)
        assert nan[:, 0].any() and not nan[:, 3:].any() and np.all(cd.C_ul[~nan] > 0)  # NaN at the cool end only
    # both "previous" inputs move between the two updates
    for c in cases.values():
        (_, n0, first), (beta, n1, second) = c["updates"]
        assert not np.array_equal(n0, n1) and beta.min() < 1e-3
        assert not np.array_equal(first["relative_populations"], second["relative_populations"])
    # the level no line reaches: singular without collision data, solved with the pairs that reach it
    with pytest.raises(nref.NlteSolveError) as e:
        nref.solve(reached["pd"], reached["ld"], reached["nd"], reached["t_rad"], reached["w"], reached["j"])
    assert (e.value.species, e.value.shell, e.value.step) == (3, 0, 16)
    a = int(reached["cd"].species_pair_edge[3])
    own = slice(a, int(reached["cd"].species_pair_edge[4]))
    touching = (reached["cd"].level_lower[own] == 9) | (reached["cd"].level_upper[own] == 9)
    assert touching.sum() == 16 and np.all(reached["updates"][0][2]["relative_populations"] > 0)
    # pair_fraction 0 everywhere: valid data without a pair
    none = synthetic.make_nlte_collision_data(13, four["pd"], four["nd"], pair_fraction=0.0)
    assert len(none.level_lower) == 0 and none.C_ul.shape == (0, 12) and _check(none, four["pd"], four["nd"])[0] == 0
