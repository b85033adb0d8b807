"""The exchange's wire conversions: gvt_hip_queues_export_wire / _append_wire (all the queues of a message in one launch) against the
per-queue loop of gvt_hip_queue_export / _append, about 1 M rays in 8 and in 64 queues of uneven sizes, exported and appended back in turn.
Per direction: wall time around calls that end in a stream synchronise (median of 30) and, in a pass of its own with gvt_hip_profile on,
the event time of the conversion kernels alone; rates in WIRE bytes (80 per ray) per second.  bytes_ok: the exported image equals the
source buffer.  EXPERIMENTS.md, "wire pair"."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gravit_amd import capi  # noqa: E402
from gravit_amd.adapter import RayQueue, queues_append_wire, queues_export_wire  # noqa: E402

capi.init(0)
dev = torch.device("cuda", 0)
TOTAL = 1 << 20
REPS = 30


def med(xs):
    return float(np.median(xs))


def run(nq, mode):
    os.environ["GVT_WIRE_LDS"] = "1" if mode == "lds" else "0"
    rng = np.random.default_rng(nq)
    w = rng.random(nq) + 0.5
    sizes = np.maximum(1, (w / w.sum() * TOTAL).astype(np.int64))
    total = int(sizes.sum())
    src = torch.randint(0, 255, (total, 80), dtype=torch.uint8, device=dev)
    buf = torch.empty((total, 80), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    queues = [RayQueue(int(s)) for s in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    queues_append_wire(queues, src.data_ptr(), [int(s) for s in sizes])
    capi.synchronize()
    t_exp, t_app, k_exp, k_app = [], [], [], []
    for rep in range(REPS + 5):
        capi.stats_reset()
        t0 = time.perf_counter()
        if mode == "loop":
            for q, o, s in zip(queues, offs, sizes):
                q.export_device(buf.data_ptr() + int(o) * 80, int(s))
                q.clear()
        else:
            queues_export_wire(queues, buf.data_ptr(), total)
        capi.synchronize()
        t1 = time.perf_counter()
        ke = capi.stats()["ms_convert"]
        capi.stats_reset()
        t2 = time.perf_counter()
        if mode == "loop":
            for q, o, s in zip(queues, offs, sizes):
                q.append_device(buf.data_ptr() + int(o) * 80, int(s))
        else:
            queues_append_wire(queues, buf.data_ptr(), [int(s) for s in sizes])
        capi.synchronize()
        t3 = time.perf_counter()
        ka = capi.stats()["ms_convert"]
        if rep >= 5:
            t_exp.append((t1 - t0) * 1e3); t_app.append((t3 - t2) * 1e3); k_exp.append(ke); k_app.append(ka)
    torch.cuda.synchronize()
    ok = bool((buf == src).all())
    gb = total * 80 / 1e9
    print("queues %3d  %-6s rays %d  export wall %.3f ms (%.0f GB/s) kernel %.3f ms (%.0f GB/s)   append wall %.3f ms (%.0f GB/s) kernel %.3f ms (%.0f GB/s)  bytes_ok %s"
          % (nq, mode, total, med(t_exp), gb / med(t_exp) * 1e3, med(k_exp), gb / max(med(k_exp), 1e-9) * 1e3, med(t_app), gb / med(t_app) * 1e3, med(k_app),
             gb / max(med(k_app), 1e-9) * 1e3, ok), flush=True)


capi.profile(1)
for nq in (8, 64):
    for mode in ("batched", "loop", "batched", "loop"):
        run(nq, mode)
capi.profile(0)
for nq in (8, 64):  # wall time without the event pairs
    for mode in ("batched", "loop", "batched", "loop"):
        run(nq, mode)
