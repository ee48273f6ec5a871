"""bench.py --dump-outputs without a GPU: the sampling and the checksums of dump_outputs() on a
stand-in for the context (the GPU run is tests/test_gpu_bench_plain.py)."""
import os

import numpy as np


def test_dump_sample_is_fixed_and_checksums_cover_everything():
    """Above DUMP_SAMPLE events the per-event arrays are written at a seeded sample: the same rows
    every time, within the 64 MB the option may write, and `checksums` still sees a change at a
    row outside the sample."""
    import bench

    class Fake:
        def __init__(self, E, flip=None):
            self.E, self.flip = E, flip

        def rounds(self):
            rnd = (np.arange(self.E) // 3500).astype(np.int32)
            if self.flip is not None:
                rnd[self.flip] += 1
            return rnd, np.zeros(self.E, np.int8), np.zeros(self.E, np.int8)

        def received(self):
            return np.ones(self.E, np.int32), np.arange(self.E, dtype=np.int64) + (3 << 60)

        def ConsensusEvents(self, g):
            return np.arange(self.E, dtype=np.int64)[::-1].copy()

        def LastConsensusRound(self, g):
            return None

        def Blocks(self, g):
            return []

        LastRound = LastCommitedRoundEvents = ConsensusTransactions = lambda self, g: 0

    import tempfile
    E = 10_000_000
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        ra = bench.dump_outputs(Fake(E), 1, a)
        assert ra["bytes"] <= 64 * 1000 * 1000
        ev = np.load(os.path.join(a, "event_sample.npy")).astype(np.int64)
        assert len(ev) == bench.DUMP_SAMPLE and np.all(np.diff(ev) > 0) and 0 <= ev[0] and ev[-1] < E
        hi = np.load(os.path.join(a, "consensus_timestamp_hi32.npy")).astype(np.int64)
        lo = np.load(os.path.join(a, "consensus_timestamp_lo32.npy")).astype(np.int64)
        assert np.array_equal((hi << 32) | lo, ev + (3 << 60))       # int64 timestamps survive exactly
        outside = int(np.setdiff1d(np.arange(1000), ev)[0])
        bench.dump_outputs(Fake(E, flip=outside), 1, b)
        for name in ra["arrays"]:
            same = np.array_equal(np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy")))
            assert same == (name != "checksums"), name
