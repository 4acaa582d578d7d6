"""The host's decisions of the blocked form of the NLTE solve as pure functions (nlte::choose_form, nlte::plan_blocked,
tardis_amd/csrc/nlte_plan.hpp), pinned without a GPU through an extern "C" shim compiled with the host C++ compiler (-Wall -Werror), in
the manner of tests/test_nlte_plan.py.  The expected values are worked out here from the header's stated rules: a species that fits the
LDS (up to 141 levels) is never blocked; of the others those at or above the threshold are; the blocked set is eliminated in
ceil(max n / NB) panel steps; step t (c0 = t NB) launches (blocked species, shells) panel workgroups and (strips, blocked species,
shells) trailing workgroups, strips being the most any species has left: ceil((n - min(n, c0 + NB) + 1) / TN), b being one more column.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tardis_amd", "csrc")

SHIM = r"""
#include "nlte_plan.hpp"
extern "C" int form_shim(long long levels, long long lds_threshold, long long blocked_threshold) { return nlte::choose_form(levels, lds_threshold, blocked_threshold); }
extern "C" int path_shim(long long levels) { return nlte::choose_path(levels); }
// out: {NB, TN, TM, BLOCKED_FORM_LEVELS, FORM_LDS, FORM_GLOBAL, FORM_BLOCKED}
extern "C" void constants_shim(long long *out)
{
    out[0] = nlte::PANEL_COLUMNS; out[1] = nlte::TILE_COLUMNS; out[2] = nlte::TILE_ROWS; out[3] = nlte::BLOCKED_FORM_LEVELS;
    out[4] = nlte::FORM_LDS; out[5] = nlte::FORM_GLOBAL; out[6] = nlte::FORM_BLOCKED;
}
// counts: {single, blocked, steps}; steps: {panel_x, panel_y, trailing_x, trailing_y, trailing_z} each; plan_out: {entries of the
// list, launches, scratch doubles} of plan_launches, its list and slabs in plan_list / plan_slab; returns 0, or 1 where cap is too small
extern "C" int blocked_shim(const int *levels, int n_species, long long n_shells, long long lds_threshold, long long blocked_threshold, int cap,
                            int *single, long long *single_slab, int *blocked, long long *blocked_slab, long long *steps, long long *counts,
                            int *plan_list, long long *plan_slab, long long *plan_out)
{
    const std::vector<int> lv(levels, levels + n_species);
    const nlte::LaunchPlan p = nlte::plan_launches(lv, n_shells, lds_threshold);
    const nlte::BlockedPlan b = nlte::plan_blocked(p, lv, n_shells, blocked_threshold);
    if ((int)p.list.size() > cap || (int)b.steps.size() > cap || b.single.size() != b.single_slab.size() || b.blocked.size() != b.blocked_slab.size()) return 1;
    for (size_t i = 0; i < b.single.size(); ++i) { single[i] = b.single[i]; single_slab[i] = b.single_slab[i]; }
    for (size_t i = 0; i < b.blocked.size(); ++i) { blocked[i] = b.blocked[i]; blocked_slab[i] = b.blocked_slab[i]; }
    for (size_t i = 0; i < b.steps.size(); ++i) {
        steps[5 * i] = b.steps[i].panel_x; steps[5 * i + 1] = b.steps[i].panel_y; steps[5 * i + 2] = b.steps[i].trailing_x;
        steps[5 * i + 3] = b.steps[i].trailing_y; steps[5 * i + 4] = b.steps[i].trailing_z;
    }
    counts[0] = (long long)b.single.size(); counts[1] = (long long)b.blocked.size(); counts[2] = (long long)b.steps.size();
    for (size_t i = 0; i < p.list.size(); ++i) { plan_list[i] = p.list[i]; plan_slab[i] = p.slab[i]; }
    plan_out[0] = (long long)p.list.size(); plan_out[1] = (long long)p.launches.size(); plan_out[2] = p.scratch_doubles;
    return 0;
}
"""

COUNTS = [3, 142, 40, 8, 9, 200, 141]


def work_doubles(n, shells):
    return shells * ((n | 1) * n + 4 * n)


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("nlte_blocked_plan")
    src = d / "nlte_blocked_plan_shim.cpp"
    src.write_text(SHIM)
    so = d / "nlte_blocked_plan_shim.so"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    ll, pi = ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)
    pll = ctypes.POINTER(ll)
    lib.form_shim.argtypes, lib.form_shim.restype = [ll, ll, ll], ctypes.c_int
    lib.path_shim.argtypes, lib.path_shim.restype = [ll], ctypes.c_int
    lib.constants_shim.argtypes, lib.constants_shim.restype = [pll], None
    lib.blocked_shim.argtypes = [pi, ctypes.c_int, ll, ll, ll, ctypes.c_int, pi, pll, pi, pll, pll, pll, pi, pll, pll]
    lib.blocked_shim.restype = ctypes.c_int
    out = (ll * 7)()
    lib.constants_shim(out)
    lib.constants = dict(zip(("NB", "TN", "TM", "BLOCKED_FORM_LEVELS", "FORM_LDS", "FORM_GLOBAL", "FORM_BLOCKED"), out))

    def blocked(levels, shells, lds_threshold=-1, blocked_threshold=-1):
        cap = 4 * len(levels) + 64
        mk_i, mk_l = (lambda k=1: (ctypes.c_int * (cap * k))()), (lambda k=1: (ll * (cap * k))())
        single, blk, plist = mk_i(), mk_i(), mk_i()
        single_slab, blk_slab, pslab, steps, counts, pout = mk_l(), mk_l(), mk_l(), mk_l(5), (ll * 3)(), (ll * 3)()
        assert lib.blocked_shim((ctypes.c_int * max(1, len(levels)))(*levels), len(levels), shells, lds_threshold, blocked_threshold, cap, single,
                                single_slab, blk, blk_slab, steps, counts, plist, pslab, pout) == 0
        a, b, t = counts
        return dict(single=list(single[:a]), single_slab=list(single_slab[:a]), blocked=list(blk[:b]), blocked_slab=list(blk_slab[:b]),
                    steps=[tuple(steps[5 * i:5 * i + 5]) for i in range(t)], list=list(plist[:pout[0]]), slab=list(pslab[:pout[0]]),
                    launches=pout[1], scratch_doubles=pout[2])

    lib.blocked = blocked
    return lib


def test_header_stays_free_of_hip():
    text = open(os.path.join(CSRC, "nlte_plan.hpp")).read()
    assert all(ln.split()[1].startswith("<") for ln in text.splitlines() if ln.startswith("#include"))
    assert "__global__" not in text and "__device__" not in text and "hipError_t" not in text


def test_choose_form_on_both_sides_of_each_threshold(shim):
    c = shim.constants
    lds, glob, blk = c["FORM_LDS"], c["FORM_GLOBAL"], c["FORM_BLOCKED"]
    assert (lds, glob, blk) == (0, 1, 2) and c["NB"] == 32
    rule = c["BLOCKED_FORM_LEVELS"]
    assert rule >= 142  # what fits the LDS is never blocked, so a smaller constant would say nothing
    form = shim.form_shim
    # the rule: 141 levels fit the LDS, 142 do not
    assert form(141, -1, -1) == lds and form(1, -1, -1) == lds
    assert form(142, -1, -1) == (blk if rule <= 142 else glob)
    assert form(rule, -1, -1) == blk and form(rule + 1, -1, -1) == blk
    if rule > 142:
        assert form(rule - 1, -1, -1) == glob
    # the blocked threshold itself, on species that are not in LDS
    assert form(199, -1, 200) == glob and form(200, -1, 200) == blk and form(142, -1, 0) == blk
    # a species in LDS is never blocked, whatever the blocked threshold says
    assert form(141, -1, 0) == lds and form(70, -1, 10) == lds
    # the LDS threshold moves species out of LDS; then the blocked threshold decides
    assert form(17, 18, 0) == lds and form(18, 18, 0) == blk and form(18, 18, 19) == glob and form(19, 18, 19) == blk
    assert form(1, 0, 0) == blk and form(1, 0, 2) == glob and form(70, 0, -1) == (blk if rule <= 70 else glob)
    # a species that does not fit the LDS leaves it whatever the LDS threshold says
    assert form(142, 1000, 0) == blk and form(142, 1000, 143) == glob


def test_the_path_of_a_blocked_species_is_still_global(shim):
    assert shim.path_shim(1071) == 1 and shim.path_shim(142) == 1 and shim.path_shim(141) == 0


def expected_steps(c, blocked_levels, shells):
    nb, tn = c["NB"], c["TN"]
    steps = []
    for t in range(ceil_div(max(blocked_levels), nb)):
        c0 = t * nb
        strips = max(ceil_div(n - min(n, c0 + nb) + 1, tn) if n > c0 else 0 for n in blocked_levels)
        steps.append((len(blocked_levels), shells, strips, len(blocked_levels), shells))
    return steps


def test_plan_blocked_under_a_threshold_of_150(shim):
    """The global launch of COUNTS holds species 1 (142 levels) and 5 (200 levels), slabs as plan_launches assigned them; from 150
    levels on blocked: 142 stays with one workgroup, 200 is eliminated in ceil(200 / NB) steps."""
    c = shim.constants
    p = shim.blocked(COUNTS, 2, -1, 150)
    assert p["list"] == [0, 3, 4, 2, 6, 1, 5] and p["launches"] == 5  # plan_launches answers as tests/test_nlte_plan.py pins it
    assert p["slab"] == [0, 0, 0, 0, 0, 0, work_doubles(142, 2)] and p["scratch_doubles"] == work_doubles(142, 2) + work_doubles(200, 2)
    assert p["single"] == [1] and p["single_slab"] == [0]
    assert p["blocked"] == [5] and p["blocked_slab"] == [work_doubles(142, 2)]
    assert p["steps"] == expected_steps(c, [200], 2) and len(p["steps"]) == ceil_div(200, c["NB"])
    if (c["NB"], c["TN"]) == (32, 32):  # by hand: 169 columns and b right of the first panel, b alone behind the last (200 = 6 x 32 + 8)
        assert [s[2] for s in p["steps"]] == [6, 5, 4, 3, 2, 1, 1]


def test_plan_blocked_with_every_species_out_of_lds(shim):
    """nlte_lds_levels = 0 and nlte_blocked_levels = 0: all seven species blocked, in index order, each with its slab."""
    c = shim.constants
    p = shim.blocked(COUNTS, 3, 0, 0)
    assert p["single"] == [] and p["blocked"] == list(range(7))
    sizes = [work_doubles(n, 3) for n in COUNTS]
    assert p["blocked_slab"] == [sum(sizes[:i]) for i in range(7)] == p["slab"] and p["scratch_doubles"] == sum(sizes)
    assert p["steps"] == expected_steps(c, COUNTS, 3) and len(p["steps"]) == ceil_div(200, c["NB"])
    # the split of the two thresholds: 9 levels and more leave the LDS, 141 and more of those are blocked
    p = shim.blocked(COUNTS, 3, 9, 141)
    assert p["single"] == [2, 4] and p["blocked"] == [1, 5, 6] and p["list"] == [0, 3, 1, 2, 4, 5, 6]
    slab = dict(zip(p["list"][2:], p["slab"][2:]))
    assert p["single_slab"] == [slab[2], slab[4]] and p["blocked_slab"] == [slab[1], slab[5], slab[6]]
    assert p["steps"] == expected_steps(c, [142, 200, 141], 3)


def test_plan_blocked_under_the_rule_and_without_a_global_launch(shim):
    c = shim.constants
    p = shim.blocked(COUNTS, 2)
    want = [sp for sp in (1, 5) if COUNTS[sp] >= c["BLOCKED_FORM_LEVELS"]]
    assert p["blocked"] == want and p["single"] == [sp for sp in (1, 5) if sp not in want]
    assert p["steps"] == (expected_steps(c, [COUNTS[sp] for sp in want], 2) if want else [])
    p = shim.blocked([3, 40, 141], 20)
    assert p["single"] == [] and p["blocked"] == [] and p["steps"] == []
    p = shim.blocked([], 20, 0, 0)
    assert p["single"] == [] and p["blocked"] == [] and p["steps"] == [] and p["list"] == []


def test_a_single_level_and_a_full_last_panel(shim):
    """n = 1: one step, b the only trailing column.  n = 64: two full panels; behind the second only b is left."""
    c = shim.constants
    assert (c["NB"], c["TN"]) == (32, 32)  # (worked out by hand for panels and strips of 32 columns)
    assert shim.blocked([1], 5, 0, 0)["steps"] == [(1, 5, 1, 1, 5)]
    assert shim.blocked([64], 5, 0, 0)["steps"] == [(1, 5, 2, 1, 5), (1, 5, 1, 1, 5)]
    assert shim.blocked([65, 33], 1, 0, 0)["steps"] == [(2, 1, 2, 2, 1), (2, 1, 1, 2, 1), (2, 1, 1, 2, 1)]
