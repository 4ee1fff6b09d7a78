"""Host-only pieces of bench.py (no GPU, no library): the flag-wait percentile summary and the watchdog around the RCCL check of the multi-GPU line, and --dump-outputs."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench


def test_wait_percentiles_reads_log2_bins_of_10ns_ticks():
    h = np.zeros((2, 2, 32), np.uint32)
    h[0, 0, 6] = 90          # [0.64, 1.28) us
    h[1, 1, 7] = 9           # [1.28, 2.56) us
    h[0, 1, 12] = 1          # [40.96, 81.92) us
    p = bench.wait_percentiles(h)
    assert p["n"] == 100 and p["p50_us"] == 1.28 and p["p90_us"] == 1.28 and p["p99_us"] == 2.56 and p["max_us"] == 81.92
    assert bench.wait_percentiles(np.zeros((2, 2, 32), np.uint32)) == {"n": 0}


def test_guarded_returns_results_reports_hangs_and_swallows_exceptions():
    assert bench.guarded(lambda: 7, 5.0) == (7, False)
    r, alive = bench.guarded(lambda: time.sleep(3.0), 0.2)
    assert r is None and alive
    r, alive = bench.guarded(lambda: 1 / 0, 5.0)
    assert r is None and not alive


class _Net:
    def __init__(self, n, seed):
        self.p = np.random.default_rng(seed).standard_normal(n).astype(np.float32)

    def get_params(self):
        return self.p.copy()

    def adam_state(self):
        return self.p * 0.5, self.p * self.p, np.array([0.9 ** 3, 0.999 ** 3])


class _Buf:
    """the host side of ExperienceBuffer that bench.dump_outputs reads: len, keys, buf[k] -> (rows, n) in the library's dtypes"""
    def __init__(self, n):
        r = np.random.default_rng(1)
        self.cols = {"s": r.standard_normal((17, n)).astype(np.float32), "a": r.random((2, n)) < 0.5, "done": r.random((1, n)) < 0.01,
                     "advantage": r.standard_normal((1, n)).astype(np.float32), "t": r.integers(0, 1000, (1, n))}

    def __len__(self):
        return self.cols["s"].shape[1]

    def keys(self):
        return list(self.cols)

    def __getitem__(self, k):
        return self.cols[k]


def test_dump_outputs_writes_float_arrays_a_fixed_sample_and_stays_under_64_mb(tmp_path):
    class _Pi:
        A, C = _Net(4610, 2), _Net(4545, 3)
    buf = _Buf(262144)                                      # the C5 shard's buffer: more rows than are written
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    info, ti = {"sum_r": 12.5, "n_episode_end": 3, "avg_r": float("nan")}, {"actor_loss": -0.01, "actor_batches_trained": 40960, "note": "text", "x": None}
    total = bench.dump_outputs(d1, _Pi, buf, info, ti)
    bench.dump_outputs(d2, _Pi, buf, info, ti)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and 0 < total <= 64 << 20
    assert {"actor_params.npy", "critic_adam_v.npy", "buffer_s.npy", "buffer_rows.npy", "rollout_info_sum_r.npy", "train_info_actor_loss.npy"} <= set(names)
    assert "train_info_note.npy" not in names and "train_info_x.npy" not in names
    for n in names:
        a, b = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), n
    rows = np.load(os.path.join(d1, "buffer_rows.npy")).astype(np.int64)
    assert rows.size == bench.DUMP_MAX_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(os.path.join(d1, "buffer_s.npy")), buf.cols["s"][:, rows])
    assert np.array_equal(np.load(os.path.join(d1, "buffer_t.npy")), buf.cols["t"][:, rows].astype(np.float64))
    assert np.array_equal(np.load(os.path.join(d1, "actor_params.npy")), _Pi.A.p)
    small = _Buf(1000)                                      # a buffer within the limit is written whole
    bench.dump_outputs(str(tmp_path / "c"), _Pi, small, {}, {})
    assert np.array_equal(np.load(str(tmp_path / "c" / "buffer_advantage.npy")), small.cols["advantage"])
