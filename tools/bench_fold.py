"""Fold rates, HBM-resident, one JSON line per measurement (dev tool; results under profiles/).

    python tools/bench_fold.py [--samples 262144] [--window 1.0] [--repeats 5]

(a) Fold of a float32 (samples, 1024, 4) stream in HBM, step=None, n_phase 64 / 256 / 1024,
    next to Integrate(ds, 16) on the same stream (k_detect_integrate).
(c) host time per call of the run table, next to the device time of the same call.
Each rate is warm, over a window of at least ``--window`` seconds, repeated ``--repeats``
times (median and spread reported).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baseband_tasks_amd as bt          # noqa: E402

T0 = bt.Time('2020-01-01T00:00:00')


def rate(make, n_samples, window, repeats):
    """Input samples per second of ``make().read_device()`` (fresh task per call: no cache)."""
    make().read_device()
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeats):
        n, t0 = 0, time.perf_counter()
        while True:
            make().read_device()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= window:
                break
        rates.append(n * n_samples / dt)
    return float(np.median(rates)), float(min(rates)), float(max(rates))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=1 << 18)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    bt.hip.set_stream(torch.cuda.current_stream().cuda_stream)
    n, fs = args.samples, 1e6
    x = torch.rand((n, 1024, 4), device='cuda', dtype=torch.float32)
    ds = bt.DeviceStream(x, T0, fs)
    gbytes = n * 1024 * 4 * 4 / 1e9
    med, lo, hi = rate(lambda: bt.Integrate(ds, 16), n, args.window, args.repeats)
    base = med
    print(json.dumps(dict(what='integrate16', samples=n, rate=med, min=lo, max=hi,
                          gb_per_s=med * gbytes / n)), flush=True)
    for n_phase in (64, 256, 1024):
        ph = (lambda t: 0.1 + 20.3 * (t - T0))          # (about 5 cycles over the stream)
        med, lo, hi = rate(lambda: bt.Fold(ds, n_phase, ph), n, args.window, args.repeats)
        fh = bt.Fold(ds, n_phase, ph)
        t0 = time.perf_counter()
        fh._counts(0, 1)
        host = time.perf_counter() - t0
        print(json.dumps(dict(what='fold', n_phase=n_phase, samples=n, rate=med, min=lo, max=hi,
                              gb_per_s=med * gbytes / n, vs_integrate=med / base,
                              host_table_s=host, device_call_s=n / med)), flush=True)


if __name__ == '__main__':
    main()
