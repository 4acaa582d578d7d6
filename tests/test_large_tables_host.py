"""The 64-bit table offsets' query is bound (include/tardis_mc.h, _lib.SYMBOLS, Engine)."""
import os

import pytest

from tardis_amd import _lib
from tardis_amd.engine import Engine


def test_symbol_is_declared_and_bound():
    assert "tardis_mc_last_table_offsets" in _lib.SYMBOLS
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "tardis_mc.h")) as f:
        assert "int tardis_mc_last_table_offsets(TardisMcContext *ctx);" in f.read()
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("engine library not built")
    L = _lib.lib()
    assert L.tardis_mc_last_table_offsets(None) == -1


def test_engine_method():
    assert callable(getattr(Engine, "last_table_offsets", None))
