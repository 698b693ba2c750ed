"""Fold rates, HBM-resident, one JSON line per measurement (dev tool; results under profiles/).

    python tools/bench_fold.py [--samples 262144] [--window 1.0] [--repeats 5] [--msp]

(a) Fold of a float32 (samples, 1024, 4) stream in HBM, step=None, n_phase 64 / 256 / 1024,
    next to Integrate(ds, 16) on the same stream (k_detect_integrate).
(c) host time per call of the run table, next to the device time of the same call.
(d) with --msp: a millisecond pulsar at the raw rate -- 2^26 float32 samples of two streams at
    16 MHz, 1024 bins, the 1.56 ms period of tests/golden/B1937_polyco.dat -- with the run table
    made by the phase callable alone (a lambda around the `PolycoPhase`: the crossing search of
    `fold_table.bin_runs`), by NumPy from the polynomial pieces (every sample), and by the table
    kernel; per route the time of one table and the rate of the whole `Fold`.
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


def millisecond_pulsar(window, repeats, n=1 << 26, fs=16e6, n_phase=1024):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pp = bt.phases.PolycoPhase(os.path.join(root, 'tests', 'golden', 'B1937_polyco.dat'))
    t0 = bt.Time('2018-05-06T22:20:00')
    x = torch.rand((n, 2), device='cuda', dtype=torch.float32)
    ds = bt.DeviceStream(x, t0, fs)
    routes = (('device', pp, 'device'), ('host', pp, 'host'), ('callable', (lambda t: pp(t)), None))
    for name, phase, route in routes:
        def make():
            fh = bt.Fold(ds, n_phase, phase)
            fh.table_route = route
            return fh
        edges, table = make()._tables(0, 1)
        table(int(edges[0]), int(edges[-1]))                       # warm
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            t = time.perf_counter()
            table(int(edges[0]), int(edges[-1]))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        med, lo, hi = rate(make, n, window, repeats)
        print(json.dumps(dict(what='fold_msp', route=name, samples=n, sample_rate=fs, n_phase=n_phase,
                              table_s=float(np.median(times)), table_s_min=min(times), table_s_max=max(times),
                              rate=med, min=lo, max=hi, fold_call_s=n / med)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=1 << 18)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--msp', action='store_true', help='the raw-rate millisecond-pulsar case only')
    args = ap.parse_args()
    bt.hip.set_stream(torch.cuda.current_stream().cuda_stream)
    if args.msp:
        millisecond_pulsar(args.window, args.repeats)
        return
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
