"""Full r-packet tracking, host side: the CSR container, the TrackerFull filler and the C struct (no GPU)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tardis_amd import _abi, transport
from tardis_amd import state as st


def _log():
    offsets = np.array([0, 3, 3, 5])
    n = 5
    cols = {f: np.arange(n, dtype=np.float64) + 0.5 for f in st.FullTrackers.F64_FIELDS}
    cols.update({f: np.arange(n, dtype=np.int64) for f in st.FullTrackers.I64_FIELDS})
    cols["event_id"] = np.array([0, 1, 2, 0, 1])
    cols["interaction_type"] = np.array([1, 2, 4, 2, 1])
    cols["status"] = np.array([0, 0, 1, 0, 2])
    cols["line_absorb_id"] = np.array([-1, 7, -1, 9, -1])
    return st.FullTrackers(offsets, cols)


def test_offsets_and_slices():
    log = _log()
    assert len(log) == 3 and log.n_rows == 5
    assert np.array_equal(log.counts, [3, 0, 2])
    assert np.array_equal(log.packet_id, [0, 0, 0, 2, 2])
    p2 = log.packet(2)
    assert np.array_equal(p2["event_id"], [0, 1]) and np.array_equal(p2["radius"], [3.5, 4.5])
    assert np.shares_memory(p2["radius"], log.radius)  # views, not copies
    assert len(log.packet(1)["shell_id"]) == 0
    assert np.array_equal(log.packet(-1)["status"], [0, 2])
    with pytest.raises(IndexError):
        log.packet(3)
    with pytest.raises(ValueError):
        st.FullTrackers([1, 2])
    with pytest.raises(ValueError):
        st.FullTrackers([0, 2], {"radius": np.zeros(3)})


def test_dataframe_index_columns_and_dtypes():
    df = _log().to_dataframe()
    assert df.index.names == ["packet_id", "event_id"]
    assert list(df.index) == [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1)]
    assert list(df.columns) == ["interaction_type", "status", "shell_id", "after_shell_id", "radius", "before_nu", "before_mu",
                                "before_energy", "after_nu", "after_mu", "after_energy", "line_absorb_id", "line_emit_id"]
    assert isinstance(df["interaction_type"].dtype, pd.CategoricalDtype)
    assert list(df["interaction_type"].dtype.categories) == ["NO_INTERACTION", "BOUNDARY", "LINE", "ESCATTERING", "CONTINUUM_PROCESS"]
    assert list(df["interaction_type"].astype(str)) == ["BOUNDARY", "LINE", "ESCATTERING", "LINE", "BOUNDARY"]
    assert list(df["status"].dtype.categories) == ["IN_PROCESS", "EMITTED", "REABSORBED", "ADIABATIC_COOLING"]
    assert list(df["status"].astype(str)) == ["IN_PROCESS", "IN_PROCESS", "EMITTED", "IN_PROCESS", "REABSORBED"]
    assert df["radius"].dtype == np.float64 and df["shell_id"].dtype == np.int64
    assert df["line_absorb_id"].dtype == np.int64 and list(df["line_absorb_id"]) == [-1, 7, -1, 9, -1]


class _TrackerFull:
    def __init__(self, extra=None):
        self.r = np.zeros(8)
        self.shell_id = np.zeros(8, dtype=np.int64)
        self.interaction_type = np.zeros(8, dtype=np.int64)
        self.after_nu = np.zeros(8)
        self.interaction_line_absorb_id = np.zeros(8, dtype=np.int64)
        self.interactions_count = 0
        if extra:
            setattr(self, extra, np.zeros(8))

    def finalize(self):  # (methods are left alone)
        raise AssertionError("not called")


def test_fill_full_trackers_by_name_and_truncation():
    log = _log()
    trackers = [_TrackerFull() for _ in range(3)]
    transport._fill_full_trackers(trackers, log)
    assert [t.interactions_count for t in trackers] == [3, 0, 2]
    assert np.array_equal(trackers[0].r, [0.5, 1.5, 2.5]) and trackers[0].r.dtype == np.float64
    assert np.array_equal(trackers[2].interaction_type, [2, 1]) and trackers[2].interaction_type.dtype == np.int64
    assert np.array_equal(trackers[2].interaction_line_absorb_id, [9, -1])
    assert np.array_equal(trackers[2].after_nu, [3.5, 4.5])
    assert len(trackers[1].shell_id) == 0
    assert transport._is_full_trackers(trackers)
    assert not transport._is_full_trackers(st.LastInteractionTrackers(3))
    with pytest.raises(ValueError):
        transport._fill_full_trackers(trackers[:2], log)


def test_fill_full_trackers_names_an_unknown_field():
    with pytest.raises(NotImplementedError, match="photon_weight"):
        transport._fill_full_trackers([_TrackerFull("photon_weight") for _ in range(3)], _log())


def test_event_log_struct_is_pinned():
    assert C.sizeof(_abi.TardisMcEventLog) == 144
    names = [f[0] for f in _abi.TardisMcEventLog._fields_]
    assert names[:4] == ["capacity", "count", "dropped", "offsets"]
    assert len(names) == 18


def test_solver_rejects_resident_full_tracking():
    solver = transport.MCTransportSolverHIP(np.linspace(1e14, 1e16, 11), resident=True, enable_rpacket_tracking=True)
    assert solver.enable_rpacket_tracking
    ts = transport.MonteCarloTransportState(None, None, None, 1.0)
    with pytest.raises(NotImplementedError, match="enable_rpacket_tracking"):
        solver.run(ts)
