"""The tabular rows and the snapshot's attributes of every driver that shares the maze scaffold (dne_hip/maze_run.py, ga_gpu.py's generation helpers),
pinned against a recording: tests/golden/maze_driver_rows.json holds, per driver, the key sequence of each table dumped to log.txt and
sorted(vars(state)) of the final snapshot.pkl after two iterations on the host-function engines.  tests/golden/make_maze_driver_golden.py wrote it and
holds the runs; this test runs the same ones.  No GPU."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_maze_driver_golden", os.path.join(HERE, "golden", "make_maze_driver_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.OUT) as _f:
    RECORDED = json.load(_f)


def test_the_recording_covers_every_run():
    assert sorted(RECORDED) == sorted(G.RUNS)
    for name, rec in RECORDED.items():
        assert len(rec["tables"]) == G.ITERS and all(rec["tables"]) and rec["state"], name
    # a plain GA state carries no novelty-search attribute; the GA-NS one does
    assert not {"archive", "k", "archive_prob"} & set(RECORDED["ga_maze"]["state"])
    assert {"archive", "k", "archive_prob"} <= set(RECORDED["ga_ns_maze"]["state"])


@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_driver_logs_and_keeps_exactly_the_recorded_names(oracle, tmp_path, name):
    got = G.rows_of(name, tmp_path)
    assert got["tables"] == RECORDED[name]["tables"]
    assert got["state"] == RECORDED[name]["state"]
