"""The yardstick of the v-packet log's last-interaction columns (option vpacket_last_interaction, tardis_mc_get_vpacket_log): plain
numpy on a FULL r-packet event log, which tests/test_full_tracking_gpu.py pins to the oracle.

A packet spawns a volley of ``number_of_vpackets`` v-packets at launch and after every LINE or ESCATTERING event, each time only if its
lab-frame frequency passes ``not (nu < spawn_start or nu > spawn_end)`` (trace_vpacket_volley, virtual_packet.py:248-386).  So, for
packet p:
  - the launch volley exists if ``nu0[p]`` passes the test and contributes the EMPTY record (type = in_id = out_id = shell_id = -1,
    in_nu = in_r = NaN: the conventions of LastInteractionTrackers for a packet without an interaction);
  - in row order, one volley follows every LINE (2) or ESCATTERING (4) row whose ``after_nu`` passes the test and contributes that
    row's (before_nu, radius, type, line_absorb_id, line_emit_id, shell_id);
  - every volley contributes exactly ``number_of_vpackets`` entries.
``nu0`` is the packet's lab-frame frequency when it is launched; the first row of a packet's log holds it as ``before_nu`` (nothing
changes a packet's frequency before its first interaction, and every packet has at least one row).
"""
import numpy as np

LINE, ESCATTERING = 2, 4
INT_FIELDS = ("last_interaction_type", "last_interaction_in_id", "last_interaction_out_id", "last_interaction_shell_id")


def launch_nus(offsets, before_nu):
    """nu0 of every packet from a full event log: before_nu of its first row."""
    offsets = np.asarray(offsets)
    assert np.all(np.diff(offsets) >= 1), "every packet has at least one row"
    return np.asarray(before_nu)[offsets[:-1]]


def expected_log(offsets, interaction_type, before_nu, after_nu, radius, line_absorb_id, line_emit_id, shell_id, nu0, spawn_start,
                 spawn_end, number_of_vpackets):
    """The expected columns, as a dict: offsets [P + 1], source_packet and the six last_interaction_* columns [count], and the volley
    statistics launch_volleys / launch_skipped / interaction_volleys / interaction_skipped."""
    offsets = np.asarray(offsets, dtype=np.int64)
    P, nv = len(offsets) - 1, int(number_of_vpackets)
    itype = np.asarray(interaction_type)

    def passes(nu):
        return ~((nu < spawn_start) | (nu > spawn_end))

    packet_of_row = np.repeat(np.arange(P, dtype=np.int64), np.diff(offsets))
    interaction = (itype == LINE) | (itype == ESCATTERING)
    spawns = interaction & passes(np.asarray(after_nu))
    launch = passes(np.asarray(nu0))
    rows = np.flatnonzero(spawns)
    # volleys in (packet, time) order: the launch volley sorts before every row of its packet
    v_packet = np.concatenate([np.flatnonzero(launch), packet_of_row[rows]])
    v_row = np.concatenate([np.full(int(launch.sum()), -1, dtype=np.int64), rows])
    order = np.lexsort((v_row, v_packet))
    v_packet, v_row = v_packet[order], v_row[order]
    empty = v_row < 0
    src = np.where(empty, 0, v_row)

    def col(values, fill, dtype):
        return np.repeat(np.where(empty, fill, np.asarray(values)[src]).astype(dtype), nv)

    out = {
        "source_packet": np.repeat(v_packet, nv),
        "last_interaction_in_nu": col(before_nu, np.nan, np.float64),
        "last_interaction_in_r": col(radius, np.nan, np.float64),
        "last_interaction_type": col(itype, -1, np.int64),
        "last_interaction_in_id": col(line_absorb_id, -1, np.int64),
        "last_interaction_out_id": col(line_emit_id, -1, np.int64),
        "last_interaction_shell_id": col(shell_id, -1, np.int64),
    }
    per_packet = np.bincount(v_packet, minlength=P) * nv
    out["offsets"] = np.concatenate([[0], np.cumsum(per_packet)]).astype(np.int64)
    out.update(launch_volleys=int(launch.sum()), launch_skipped=int(P - launch.sum()), interaction_volleys=int(spawns.sum()),
               interaction_skipped=int(interaction.sum() - spawns.sum()))
    return out


def expected_from_event_log(log, spawn_start, spawn_end, number_of_vpackets):
    """``log``: anything with the columns of ``state.FullTrackers`` (offsets, interaction_type, before_nu, after_nu, radius,
    line_absorb_id, line_emit_id, shell_id)."""
    return expected_log(log.offsets, log.interaction_type, log.before_nu, log.after_nu, log.radius, log.line_absorb_id,
                        log.line_emit_id, log.shell_id, launch_nus(log.offsets, log.before_nu), spawn_start, spawn_end,
                        number_of_vpackets)


def same_bits(a, b):
    """Bit-for-bit equality of two float64 arrays up to the payload of NaN: NaN in the same places, identical bits elsewhere."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
