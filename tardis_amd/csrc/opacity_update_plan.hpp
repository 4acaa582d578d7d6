// opacity_update_plan.hpp -- which form of the block kernel of tardis_mc_update_opacity a macro-atom block takes: the host's decision as a
// pure function.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_opacity_update_host.py pins the rule through
// tardis_mc_opacity_update_path.  The kernels are in opacity_update.hpp.
//
// A block of `rows` transition rows is normalised per shell either by one lane (PATH_LANE: the lane walks the block, eight rows requested
// together) or by a 16-lane DPP row (PATH_ROW: sixteen consecutive rows per step, the additions carried in row order).  Both forms add
// in the same order, so the choice changes no bit of the result, only the time.  Measured (profiles/opacity_update.txt): the row form
// wins wherever it was tried -- its lanes read consecutive rows, the lane form's lanes read rows a block apart.  The block kernels of the
// configs[2] tables (1.5e6 rows, blocks of 12 to 18 000) take 16.6 ms with every block on a lane, 2.57 ms with the row form from 32 rows,
// 2.23 from 16, 2.12 from 8; the 12-to-24-row blocks of the tardis_example shape 0.077 / 0.057 (from 16) / 0.032 ms (from 8).  Neither shape
// has a block below 8 rows, so nothing was measured there: below half a row of lanes a block stays on one lane.
#pragma once

namespace opup {

constexpr int PATH_LANE = 0, PATH_ROW = 1;
constexpr long long LONG_BLOCK_ROWS = 8;  // blocks of this many rows or more take a 16-lane row per (block, shell)

// `threshold` < 0: the measured rule; otherwise blocks of `threshold` rows or more take the row form (option opacity_update_long_rows)
inline int choose_path(long long rows, long long threshold = -1)
{
    const long long t = threshold < 0 ? LONG_BLOCK_ROWS : threshold;
    return rows > 0 && rows >= t ? PATH_ROW : PATH_LANE;
}

}  // namespace opup
