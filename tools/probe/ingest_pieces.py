"""Step time (clear + insert_and_run32) on one context by the pipelined ingest's piece count and the
lastAncestors time segments, pageable then page-locked host columns (the numbers in
profiles/r07_ingest_pipeline/). Usage:
    python tools/probe/ingest_pieces.py [c3|c2] [pieces:segments,...] [steps]
pieces 0 = the serial order; segments 0 = the default (hgx_set_la_kernel otherwise)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from babble_amd import trace  # noqa: E402
from babble_amd.hashgraph import Hashgraph, compact_columns, pinned_columns  # noqa: E402

cfgs = {"c3": (256, 10_000_000), "c2": (64, 1 << 20)}
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
combos = [tuple(int(y) for y in x.split(":")) for x in (sys.argv[2] if len(sys.argv) > 2 else "0:0,2:0,4:0").split(",")]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
n, E = cfgs[name]
cols = compact_columns(trace.gossip(n, E, 1))
h = Hashgraph(n, capacity=E)
h.set_kernel_timing(False)
for mem in ("pageable", "pinned"):
    cc = cols if mem == "pageable" else pinned_columns(cols)
    use = {k: v for k, v in cc.items() if k != "_buffers"}
    for rnd in range(2):
        for p, la in combos:
            h.set_ingest_pipeline(p, 0)
            h.set_la_kernel(la)
            ts = []
            for i in range(reps + 2):   # two warm-up steps
                t0 = time.perf_counter()
                h.clear()
                h.insert_and_run32(use)
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = sorted(ts[2:])
            ph = h.phase_times()
            print(f"{name} {mem} round {rnd} pieces {p} la {la}: verify {ph['la_verify']} used {ph['ingest_pieces']} "
                  f"segs {ph['la_wave_segs']} min {ts[0]:.2f} med {ts[len(ts) // 2]:.2f} max {ts[-1]:.2f} "
                  f"coords {ph['coords_ms']:.2f}", flush=True)
