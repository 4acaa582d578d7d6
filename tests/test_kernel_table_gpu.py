"""Every row of the three tables of compiled propagation kernels, launched once and held against the CPU oracle.

The rows are enumerated from the library (tardis_mc_kernel_table_row), so the test ids are the table: one id per instantiation.  Each row
runs through its recipe (tests/kernel_table_recipes.py) on a fresh engine, and two things are asserted: Engine.last_kernel_key() is the
row -- the call ran on that instantiation and on no neighbour -- and its results are the oracle's, at the bars of tests/test_hip_parity.py:
per-packet results, tracker fields and v-packet log columns bit for bit, estimators within rtol 1e-11, work counters exactly.

Problem: 12 shells x 3000 lines, macro-atom with heavy-tailed blocks, 6037 packets (94 full waves and one of 21 lanes; no multiple of 8,
16 or 64), with 0 or 3 v-packets and partial or full relativity: four oracle runs, cached.  WIDE rows run at this shape with
table_offsets 1 (tables of 2^28 entries: tests/test_large_tables_gpu.py).  XWALK rows run twice, with debug flag 8192 and with 128.
"""
import time

import pytest

import kernel_table_recipes as ktr

pytestmark = pytest.mark.gpu

ROWS = [(t, row) for t in ktr.TABLES for row in ktr.table_rows(t)]


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("n_vpackets", [0, ktr.N_VPACKETS])
def test_the_sample_is_mixed(oracle, full, n_vpackets):
    """From the oracle result alone: the sample holds every class of packet, and macro-atom transitions."""
    _, ref = ktr.case(oracle, full, n_vpackets)
    mix = ktr.sample_mix(ref)
    print(full, n_vpackets, mix, "most interactions", int(ref.trackers.interactions_count.max()), "macro transitions", ref.counters["macro_transitions"])
    for what, n in mix.items():
        assert n >= 500, what
    assert ref.counters["macro_transitions"] > 0
    if n_vpackets:
        assert ref.vpacket_log_count > 1000


@pytest.mark.parametrize("table,row", ROWS, ids=[ktr.row_id(t, row) for t, row in ROWS])
def test_row(oracle, table, row):
    k = dict(zip(ktr.FIELDS[table], row))
    t0 = time.perf_counter()
    for rec in ktr.recipes(table, row) or [ktr.recipe(table, row)]:  # (no recipe: recipe() says so)
        prob, ref = ktr.case(oracle, rec.full, rec.n_vpackets)
        got = ktr.run(rec, prob, ref)
        assert got.row == (table, row), (rec.options, got.row)
        res = got.results
        ktr.same_per_packet(res, ref, trackers=bool(k["TRACK"]))
        ktr.same_estimators_and_counters(res, ref)
        if k["VPK"]:
            ktr.same_vpacket_log(res, got.vpacket_log, ref)
        if k["VLI"]:
            ktr.same_last_interaction_columns(got.vpacket_log, ktr.lane_event_log(oracle, rec.full, rec.n_vpackets), prob.montecarlo_configuration,
                                              rec.n_vpackets)
        if k.get("FT"):
            if table == "lane":
                ktr.same_as_oracle_trace(got.event_log, ktr.oracle_trace(oracle, rec.full, rec.n_vpackets), res)
            else:
                ktr.same_event_log(got.event_log, ktr.lane_event_log(oracle, rec.full, rec.n_vpackets))
    print(ktr.row_id(table, row), "%.2f s" % (time.perf_counter() - t0))
