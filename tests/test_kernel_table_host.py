"""The tables of compiled propagation kernels, enumerated from the library (tardis_mc_kernel_table_row; no GPU): no key twice, a recipe
for every row (tests/kernel_table_recipes.py), no recipe for two rows.  tests/test_kernel_table_gpu.py launches every row through its
recipe; a row added without one fails here, on the build machine."""
import ctypes as C
import os

import pytest

import kernel_table_recipes as ktr
from tardis_amd import _abi, _lib
from tardis_amd.engine import Engine


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return {t: ktr.table_rows(t) for t in ktr.TABLES}


def test_enumeration(tables):
    L = _lib.lib()
    key = (C.c_int * 12)()
    for t, name in enumerate(ktr.TABLES):
        rows = tables[name]
        n = L.tardis_mc_kernel_table_row(t, 0, None)  # (the count alone)
        assert n == len(rows) > 0
        for r, row in enumerate(rows):
            for i in range(12):
                key[i] = -7
            assert L.tardis_mc_kernel_table_row(t, r, key) == n
            width = len(ktr.FIELDS[name])
            assert tuple(key[:width]) == row and not any(key[width:]), (name, r)  # (the unused tail is zero)
        for bad in (-1, n, n + 5):  # a row outside the table: the count, the key untouched
            key[0] = -7
            assert L.tardis_mc_kernel_table_row(t, bad, key) == n and key[0] == -7
    for bad in (-1, 3, 99):
        assert L.tardis_mc_kernel_table_row(bad, 0, key) == _abi.ERR_INVALID_ARGUMENT < 0
    with pytest.raises(ValueError):
        Engine.kernel_table("volley")


def test_no_key_twice(tables):
    for name, rows in tables.items():
        seen = set()
        for row in rows:
            assert row not in seen, ktr.row_id(name, row)
            seen.add(row)


def test_every_row_has_a_recipe(tables):
    missing = []
    for name, rows in tables.items():
        for row in rows:
            found = ktr.recipes(name, row)
            if not found:
                missing.append(ktr.row_id(name, row))
                continue
            assert ktr.recipe(name, row) == found[0]
            xwalk = name == "wave" and row[ktr.FIELDS["wave"].index("XWALK")]
            assert len(found) == (2 if xwalk else 1), ktr.row_id(name, row)  # (debug flag 8192, then 128)
            for rec in found:
                assert set(rec.options) == set(ktr.OPTIONS) and rec.options["ls_waves_per_simd"] in (3, 4)
                assert ktr.selected_row(rec) == (name, row)
    assert not missing, "rows without a recipe in tests/kernel_table_recipes.py: " + ", ".join(missing)


def test_no_recipe_for_two_rows(tables):
    owner = {}
    for name, rows in tables.items():
        for row in rows:
            for rec in ktr.recipes(name, row):
                rid = ktr.recipe_id(rec)
                assert rid not in owner, (ktr.row_id(name, row), ktr.row_id(*owner[rid]))
                owner[rid] = (name, row)


def test_every_key_the_options_can_produce_is_a_row(tables):
    """The forward direction over the whole product of the family's configurations and option values: every call lands on a row of its
    table or is refused -- no key the tables lack.  (ktr.selected_row is a transcription of the host's choice functions; that it tells
    the truth for every row is what the GPU test shows.)"""
    import itertools
    values = dict(variant=(0, 1, 2, 3, 4), group_size=(0, 4, 8, 16), track_last_interaction=(0, 1), track_full=(0, 1), vpacket_last_interaction=(0, 1),
                  table_offsets=(0, 1), vpk_wide_registers=(0, 2), ls_waves_per_simd=(3, 4), sweep_table=(0, 1, 2), log_by_shell=(0, 1), est_pipeline=(0, 1),
                  debug_flags=(0, ktr.WALK_LANE_FP64, ktr.WALK_GROUP_FP64))
    assert set(values) == set(ktr.OPTIONS)
    have = {name: set(rows) for name, rows in tables.items()}
    reached = {name: set() for name in tables}
    for full, n_v in itertools.product((False, True), (0, ktr.N_VPACKETS)):
        for combo in itertools.product(*values.values()):
            rec = ktr.Recipe(full, n_v, n_v > 0, dict(zip(values, combo)))
            table, key = ktr.selected_row(rec)
            if table != "error":
                assert key in have[table], (ktr.row_id(table, key), rec)
                reached[table].add(key)
    assert reached == have  # (and nothing in the tables that the product does not reach)


def test_refused_combinations_are_not_rows():
    """What the forward direction says of option sets the library refuses: an error, never a row."""
    rec = ktr.recipe("wave", (0, 1, 16, 1, 0, 0, 3, 0, 0, 0, 0, 1))
    off = rec._replace(options=dict(rec.options, track_last_interaction=0))
    assert ktr.selected_row(off)[0] == "error"  # (vpacket_last_interaction without a tracker)
    rec = ktr.recipe("wave", (0, 1, 8, 0, 0, 1, 4, 0, 0, 0, 0, 0))
    wide = rec._replace(options=dict(rec.options, table_offsets=1))
    assert ktr.selected_row(wide)[0] == "error"  # (the cross-check instantiations have no 64-bit table offsets)
