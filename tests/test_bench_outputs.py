"""bench.py's `--dump-outputs DIR` and `--full`: the dump holds what the last timed step computed (float64, a fixed seeded
sample of the large arrays, at most 64 MB), the same in every run with the same arguments; a plain run does only what its
headline needs, `--full` adds the roofline and the other legs."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tardis_amd import state as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _StandInEngine:
    """get_results() of an engine whose every per-packet value is the packet's index and every [L,S] value the cell's flat index."""

    def __init__(self, P, L, S, n_grid=50):
        self.P, self.L, self.S, self.n_grid = P, L, S, n_grid

    def get_results(self, track_last_interaction=True, want_packet_outputs=True):
        idx = np.arange(self.P, dtype=np.float64)
        tr = None
        if track_last_interaction:
            tr = st.LastInteractionTrackers(self.P)
            for f in tr.F64_FIELDS:
                getattr(tr, f)[:] = idx
            for f in tr.I64_FIELDS:
                getattr(tr, f)[:] = np.arange(self.P)
            none = np.arange(self.P) % 7 == 3  # packets without a recorded interaction: NaN fields, as the engine leaves them
            tr.interaction_type[none] = st.INTERACTION_NONE
            for f in tr.F64_FIELDS:
                getattr(tr, f)[none] = np.nan
        cells = np.arange(self.L * self.S, dtype=np.float64).reshape(self.L, self.S)
        return types.SimpleNamespace(output_nus=idx.copy(), output_energies=-idx, trackers=tr, j_estimator=np.ones(self.S),
                                     nu_bar_estimator=np.full(self.S, 2.0), j_blue_estimator=cells, edotlu_estimator=-cells,
                                     v_packets_energy_hist=np.zeros(self.n_grid))


def test_dump_outputs_is_a_fixed_sample_within_the_size_limit(tmp_path):
    bench = _bench_module()
    pg = types.SimpleNamespace(rank=0)
    P, L, S = bench.DUMP_PACKETS + 1234, 30_000, 20  # (both above their sample sizes)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), _StandInEngine(P, L, S), pg, False, True)
    bench.dump_outputs(str(b), _StandInEngine(P, L, S), pg, False, True)
    names = sorted(f[:-4] for f in os.listdir(a))
    assert names == sorted(f[:-4] for f in os.listdir(b)) and len(names) == 2 + 14 + 5  # (outputs, trackers, estimators + v-packet histogram)
    assert "output_nus" in names and "last_interaction_interactions_count" in names and "j_blue_estimator" in names
    assert "last_interaction_mu" not in names  # (the engine does not write it)
    total = 0
    for n in names:
        x, y = np.load(a / (n + ".npy")), np.load(b / (n + ".npy"))
        assert x.dtype == np.float64 and np.array_equal(x, y), n  # the same sample in every run
        assert np.all(np.isfinite(x)), n
        total += x.nbytes
    assert total <= 64 * 2**20
    pick = np.load(a / "output_nus.npy")
    assert len(pick) == bench.DUMP_PACKETS and np.all(np.diff(pick) > 0) and pick[-1] < P  # distinct packets, in packet order
    assert np.array_equal(np.load(a / "output_energies.npy"), -pick)
    assert np.array_equal(np.load(a / "last_interaction_shell_id.npy"), pick)  # one packet sample for every per-packet array
    none = pick % 7 == 3
    assert none.any() and np.array_equal(np.load(a / "last_interaction_interaction_type.npy") == st.INTERACTION_NONE, none)
    assert np.array_equal(np.load(a / "last_interaction_radius.npy"), np.where(none, 0.0, pick))  # (no interaction recorded: 0.0)
    cells = np.load(a / "j_blue_estimator.npy")
    assert len(cells) == bench.DUMP_LINE_CELLS and np.all(np.diff(cells) > 0) and cells[-1] < L * S
    assert np.array_equal(np.load(a / "edotlu_estimator.npy"), -cells)
    assert np.array_equal(np.load(a / "j_estimator.npy"), np.ones(S))
    # the headline's shape (1e8 packets, 5e5 lines x 20 shells, tracking on) stays within the limit, too
    assert (2 + 14) * 8 * bench.DUMP_PACKETS + 2 * 8 * bench.DUMP_LINE_CELLS + 8 * (2 * 100 + 10_000) <= bench.DUMP_LIMIT_BYTES


def test_small_outputs_are_dumped_whole(tmp_path):
    bench = _bench_module()
    bench.dump_outputs(str(tmp_path), _StandInEngine(1000, 300, 5), types.SimpleNamespace(rank=0), False, False)
    assert np.array_equal(np.load(tmp_path / "output_nus.npy"), np.arange(1000.0))
    assert np.array_equal(np.load(tmp_path / "j_blue_estimator.npy"), np.arange(1500.0))
    assert not [f for f in os.listdir(tmp_path) if f.startswith("last_interaction_")]  # (--no-tracking: no trackers)


def _bench_line(*args, timeout=600):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "2", "--packets", "200000"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_and_their_dumps(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    one = _bench_line("--steps", "3", "--warmup", "1", "--dump-outputs", str(a))
    two = _bench_line("--steps", "2", "--warmup", "1", "--dump-outputs", str(b))
    for line, steps in ((one, 3), (two, 2)):
        assert line["steps"] == steps and line["metric"] == "packets/sec" and line["unit"] == "packets/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(200_000 / (line["ms_per_step"] * 1e-3), rel=1e-9)
        assert not {"roofline", "cpu_baseline", "boundary", "extra"} & line.keys()  # (a plain run: the headline only)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "output_nus.npy" in names and "last_interaction_nu.npy" in names
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float64 and x.shape == y.shape and np.all(np.isfinite(x)), n
        if n.startswith(("output_", "last_interaction_")):
            assert np.array_equal(x, y), n  # per-packet results: bit-exact from run to run
        else:
            np.testing.assert_allclose(x, y, rtol=1e-11, err_msg=n)  # sums in another order
    assert len(np.load(a / "output_nus.npy")) == 200_000 and np.all(np.load(a / "j_estimator.npy") > 0)
    full = _bench_line("--steps", "1", "--warmup", "1", "--full", "--cpu-sample", "2000", "--boundary-packets", "20000")
    assert full["roofline"]["kernel_ms"] > 0 and "error" not in full["cpu_baseline"] and "error" not in full["boundary"]
    assert full["cpu_baseline"]["per_packet_bit_exact"] is True
