#!/usr/bin/env python3
"""Record what the drivers log and keep: per driver, the key sequence of every table dumped to log.txt and sorted(vars(state)) of the final
snapshot.pkl, after two iterations on the host-function engines of the CPU tests.  Writes tests/golden/maze_driver_rows.json, which
tests/test_driver_rows_cpu.py compares the drivers against (it runs the same RUNS).  Needs the library and the oracle built; no GPU.

Usage: python tests/golden/make_maze_driver_golden.py      (on a tree whose rows are the ones to pin)
"""
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "deep-neuroevolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "maze_driver_rows.json")
ITERS = 2


def _noise(table):
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = table
    noise._engines = []
    return noise


def _es(log_dir):
    import maze_support as M
    from dne_hip import es_gpu
    exp = {"game": "maze", "model": "SimpleClassifier", "num_test_episodes": 2, "population_size": 8, "timesteps": 10 ** 9,
           "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": M.MAZE_FILE}
    es_gpu.main(log_dir, engine=M.MazeHostEngine(max_members=8), noise=_noise(M.maze_noise()), seed=4, max_iters=ITERS, **exp)


def _nses(algo_type):
    def run(log_dir):
        import maze_novelty_support as S
        import maze_support as M
        from dne_hip import nses_gpu
        exp = {"game": "maze", "model": "SimpleClassifier", "algo_type": algo_type, "population_size": 8, "timesteps": 10 ** 9,
               "novelty_search": {"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"},
               "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_sign_rank", "l2coeff": 0.005, "mutation_power": 0.02,
               "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": M.MAZE_FILE}
        nses_gpu.main(log_dir, engine=S.MazeNoveltyHostEngine(max_members=8), noise=_noise(M.maze_noise()), seed=4, max_iters=ITERS, **exp)
    return run


def _ga(novelty_search):
    def run(log_dir):
        import maze_ga_support as G
        import maze_gans_support as S
        import maze_support as M
        from dne_hip import ga_gpu
        exp = {"game": "maze", "model": "SimpleClassifier", "population_size": 10, "selection_threshold": 3, "validation_threshold": 2,
               "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 40, "mutation_power": 0.005, "timesteps": 10 ** 9,
               "maze_file": M.MAZE_FILE}
        if novelty_search:
            exp["novelty_search"] = {"k": 3, "archive_prob": 0.3}
        eng = (S.MazeGaNsHostEngine if novelty_search else G.MazeGaHostEngine)(max_members=10)
        ga_gpu.main(log_dir, engine=eng, noise=_noise(G.noise()), seed=4, max_iters=ITERS, **exp)
    return run


def _ga_atari(log_dir):
    from oracle_engine import OracleEngine
    from dne_hip import es, ga_gpu
    exp = {"game": "frostbite", "model": "Model", "num_validation_episodes": 2, "num_test_episodes": 3, "population_size": 6,
           "episode_cutoff_mode": 12, "timesteps": 10 ** 9, "validation_threshold": 2, "selection_threshold": 3, "mutation_power": 0.002}
    ga_gpu.main(log_dir, engine=OracleEngine(1), noise=es.SharedNoiseTable(count=2_500_000), seed=5, max_iters=ITERS, **exp)


def _ga_ns_dense(env, game):
    def run(log_dir):
        import dense_gans_support as S
        from dne_hip import ga_gpu
        exp = S.exp(game)                      # LinearClassifier, population 10, T = 3, V = 2, k = 3, archive_prob = 0.3
        ga_gpu.dense_ns_main(log_dir, engine=S.host_engine((env, (), "relu"), 10), noise=S.shared_noise(), seed=4, max_iters=ITERS, **exp)
    return run


def _ga_ns_atari(log_dir):
    import atari_gans_support as S
    from dne_hip import ga_gpu
    exp = S.exp()                              # Model on frostbite, population 6, T = 2, V = 2, k = 3, archive_prob = 0.3
    ga_gpu.atari_ns_main(log_dir, engine=S.AtariGaNsHostEngine(max_members=6), noise=S.shared_noise(), seed=5, max_iters=ITERS, **exp)


RUNS = {"es_maze": _es, "nses_ns": _nses("ns"), "nses_nsr": _nses("nsr"), "ga_maze": _ga(False), "ga_ns_maze": _ga(True), "ga_atari": _ga_atari,
        "ga_ns_dense_maze": _ga_ns_dense("maze", "maze"), "ga_ns_dense_cartpole": _ga_ns_dense("cartpole", "gym.CartPole-v1"),
        "ga_ns_atari": _ga_ns_atari}


def table_keys(log_path):
    """the key sequence of every table in a log.txt, in the order dumped: a table is the '| key | value |' lines between two rules"""
    tables, rows = [], None
    for line in open(log_path):
        if line.startswith("---"):
            if rows:
                tables.append(rows)
            rows = []
        elif line.startswith("|") and rows is not None:
            rows.append(line.split("|")[1].strip())
        else:
            rows = None
    return tables


def rows_of(name, log_dir):
    """{'tables': [[key, ...], ...], 'state': sorted attribute names of the final snapshot} of one driver run in log_dir"""
    from dne_hip import tabular_logger
    RUNS[name](str(log_dir))
    tabular_logger.stop()
    with open(os.path.join(str(log_dir), "snapshot.pkl"), "rb") as f:
        state = pickle.load(f)
    return {"tables": table_keys(os.path.join(str(log_dir), "log.txt")), "state": sorted(vars(state))}


if __name__ == "__main__":
    import tempfile
    import oracle
    oracle.build()
    out = {}
    for name in RUNS:
        with tempfile.TemporaryDirectory() as tmp:
            out[name] = rows_of(name, tmp)
        assert len(out[name]["tables"]) == ITERS, (name, len(out[name]["tables"]))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {k: (len(v["tables"][0]), len(v["state"])) for k, v in out.items()})
