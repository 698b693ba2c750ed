"""Time `DeviceNoiseGenerator.read_device` against what it replaces: `NoiseGenerator` on the host,
alone and with the upload, in the same run.  Appends one JSON line to profiles/noise_bench.jsonl.

    python tools/bench_noise.py [--frames 4] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import baseband_tasks_amd as bt                      # noqa: E402
from baseband_tasks_amd import hip, units as u       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=4, help='frames of 2^20 x 2 complex64 samples per read')
    ap.add_argument('--repeat', type=int, default=3)
    args = ap.parse_args()
    spf = 1 << 20
    n = args.frames * spf
    make = dict(shape=(n * (args.repeat + 1), 2), start_time='2020-01-01T00:00:00', sample_rate=16 * u.MHz,
                samples_per_frame=spf, seed=12345)
    host = bt.NoiseGenerator(**make)
    dev = bt.DeviceNoiseGenerator(**make)
    same = np.array_equal(dev.read(4096).view(np.uint8), host.read(4096).view(np.uint8))
    dev.seek(n)
    dev.read_device(n)                               # warm-up: kernels loaded, pool filled
    hip.synchronize()
    t_dev, t_host, t_up = [], [], []
    for r in range(args.repeat):
        dev.seek(r * n)
        t0 = time.perf_counter()
        dev.read_device(n)
        hip.synchronize()
        t_dev.append(time.perf_counter() - t0)
    host.seek(0)
    t0 = time.perf_counter()
    x = host.read(n)
    t_host.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    hip.DeviceArray.from_host(x)
    hip.synchronize()
    t_up.append(time.perf_counter() - t0)
    samples = n * 2
    row = dict(bench='noise', device=hip.device_name(), frames=args.frames, samples_per_frame=spf, streams=2,
               identical_first_4096=bool(same), host_frames=dev.host_frames,
               device_s=min(t_dev), device_Msamples_per_s=samples / min(t_dev) / 1e6,
               host_generate_s=min(t_host), host_Msamples_per_s=samples / min(t_host) / 1e6,
               host_upload_s=min(t_up),
               host_plus_upload_Msamples_per_s=samples / (min(t_host) + min(t_up)) / 1e6)
    print(json.dumps(row))
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'noise_bench.jsonl'), 'a') as f:
        f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
