"""The held start entry of a post-emission trace (option `sweep_start_held`, include/tardis_mc.h; ssk::MODE_START_HELD, tardis_amd/csrc/sweep_skip.hpp and the
walk / prologue / coarse step of tardis_amd/csrc/propagate_wave.hpp; the algorithm is checked on the host in tests/test_sweep_start_held_host.py) against the
CPU oracle: per-packet outputs and last-interaction trackers bit for bit, line_visits / events / macro_transitions / rng_draws exactly, J, nu_bar and the line
estimators at the suite's tolerance -- with the option 0 and 1.

The problems are the macro-atom family with heavy-tailed blocks of tests/kernel_table_recipes.py (12 shells x 3000 lines, 6037 packets) on the two rows
that carry the block skip (sixteen waves, eight loads per step; twelve waves, ten), untracked and tracked, each call held to its intended row:
    base         the family itself, with the automatic choice of hot sectors and with every block on one (walk_hot 1: every emission of the compact walk
                 that a sector decides takes the pair read; the rest of the cases run with it)
    odd          the same on 3003 lines: rows that are no multiple of 8
    clustered    the family on the line list of tests/coincident_lines.py: runs of equal lines, lines an ulp apart, inside and just outside the threshold
    downbranch, scatter   no hot-sector emission: the bit is never set, results unchanged
    epochs       a line-visit log of a fifth of the call's records: every wave is suspended several times, with lanes between emission and sweep and in coarse
                 mode with the entry held
    switched     the options switched between the calls of one context, `sweep_skip` 0 among them (the option is ignored there)
A cross-check call counts the jumps that hot sectors decided: the path is exercised thousands of times."""
import numpy as np
import pytest

import coincident_lines  # noqa: F401  (registers the "clustered" family)
import kernel_table_recipes as ktr
from tardis_amd import synthetic

pytestmark = pytest.mark.gpu

HOT_HIT = 65536  # debug flag -> counters["reserved"] (a cross-check instantiation)
_cases = {}


def _family(oracle, name):
    if name in ("base", "clustered"):
        return ktr.case(oracle, False, 0, name)
    if name not in _cases:
        kw = dict(seed=41, n_packets=ktr.N_PACKETS, n_shells=ktr.N_SHELLS, n_lines=ktr.N_LINES, line_interaction_type="macroatom", level_sizes="heavy", n_bins=2000)
        kw.update({"odd": dict(n_lines=ktr.N_LINES + 3), "downbranch": dict(line_interaction_type="downbranch"),
                   "scatter": dict(line_interaction_type="scatter", level_sizes=None)}[name])
        if kw["level_sizes"] is None:
            del kw["level_sizes"]
        prob = synthetic.make_problem(**kw)
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
        assert ref.return_code == 0
        _cases[name] = (prob, ref)
    return _cases[name]


def skip_row(wpe, track):
    #                FULL TRACK  G  VPK LS XWALK WPE NT SL FT WIDE VLI
    return ("wave", (0, int(track), 16, 0, 1, 0, wpe, 1, 0, 0, 0, 0))


def set_up(eng, prob, wpe, track, held, skip=1):
    rec = ktr.recipe(*skip_row(wpe, track))
    for name in ktr.OPTIONS:
        eng.set_option(name, rec.options[name])
    eng.set_option("sweep_skip", skip)
    eng.set_option("sweep_start_held", held)
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()


def call(eng, ref, wpe, track, skip=1):
    eng.propagate()
    eng.synchronize()
    assert eng.last_kernel_key() == skip_row(wpe, track), eng.last_kernel_key()
    assert eng.last_sweep_skip() == skip
    res = eng.get_results(track_last_interaction=bool(track))
    ktr.same_per_packet(res, ref, trackers=bool(track))  # bit for bit
    ktr.same_estimators_and_counters(res, ref)           # estimators to 1e-11; line_visits, events, macro_transitions, rng_draws exactly
    return res


def run(prob, ref, wpe, track, held, walk_hot=1, skip=1, **options):
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_option("walk_hot", walk_hot)
        for k, v in options.items():
            eng.set_option(k, v)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        set_up(eng, prob, wpe, track, held, skip)
        call(eng, ref, wpe, track, skip)
        return eng.last_kernel_times()["launches"]


ROWS = [(4, 0), (4, 1), (3, 0), (3, 1)]
ROW_IDS = ["16waves", "16waves-tracked", "12waves", "12waves-tracked"]


@pytest.mark.parametrize("held", [0, 1])
@pytest.mark.parametrize("wpe,track", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("walk_hot", [-1, 1], ids=["hot-auto", "hot-all"])
def test_heavy_blocks(oracle, walk_hot, wpe, track, held):
    prob, ref = _family(oracle, "base")
    run(prob, ref, wpe, track, held, walk_hot=walk_hot)


@pytest.mark.parametrize("held", [0, 1])
@pytest.mark.parametrize("wpe,track", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("name", ["odd", "clustered", "downbranch", "scatter"])
def test_line_lists_and_modes(oracle, name, wpe, track, held):
    prob, ref = _family(oracle, name)
    if name == "odd":
        assert len(prob.opacity_state.line_list_nu) % 8 != 0
    run(prob, ref, wpe, track, held)


@pytest.mark.parametrize("name", ["base", "odd", "clustered"])
def test_hot_sectors_decide_thousands_of_jumps(oracle, name):
    """The census of the path under test: jumps decided by hot sectors in a cross-check call of the same problem with the same tables."""
    from tardis_amd.engine import Engine
    prob, ref = _family(oracle, name)
    with Engine(0) as eng:
        eng.set_option("walk_hot", 1)
        eng.set_option("variant", 3)
        eng.set_option("debug_flags", HOT_HIT)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        res = eng.get_results(track_last_interaction=False)
    assert np.array_equal(res.output_nus, ref.output_nus)
    print(name, "jumps decided by a hot sector", res.counters["reserved"], "events", ref.counters["events"])
    assert res.counters["reserved"] > 5000


@pytest.mark.parametrize("held", [0, 1])
@pytest.mark.parametrize("wpe,track", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("name", ["base", "odd"])
def test_several_epochs(oracle, name, wpe, track, held):
    """A small log: every wave is suspended again and again, lanes between emission and sweep and in coarse mode with the start entry held."""
    prob, ref = _family(oracle, name)
    capacity = max(256 * ((ktr.N_PACKETS + 63) // 64), int(ref.counters["events"]) // 5)
    launches = run(prob, ref, wpe, track, held, log_capacity=capacity, log_chunk_records=257)
    print(name, wpe, track, held, "log capacity", capacity, "launches", launches)
    assert launches >= 2


@pytest.mark.parametrize("held", [0, 1])
@pytest.mark.parametrize("wpe,track", ROWS, ids=ROW_IDS)
def test_sweep_skip_off(oracle, wpe, track, held):
    prob, ref = _family(oracle, "base")
    run(prob, ref, wpe, track, held, skip=0)


@pytest.mark.parametrize("name", ["base", "clustered"])
def test_options_switched_between_calls_of_one_context(oracle, name):
    from tardis_amd.engine import Engine
    prob, ref = _family(oracle, name)
    with Engine(0) as eng:
        eng.set_option("walk_hot", 1)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        for wpe, track, held, skip in ((4, 1, 1, 1), (4, 1, 0, 1), (3, 0, 1, 1), (4, 0, 1, 0), (4, 0, -1, 1), (3, 1, 0, 1), (3, 1, 1, 1), (4, 0, 1, 1), (3, 0, 0, 0)):
            set_up(eng, prob, wpe, track, held, skip)
            call(eng, ref, wpe, track, skip)
