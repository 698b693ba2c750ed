"""Rates of the spectral-kurtosis kernels, one JSON line per case (dev tool).

    python tools/bench_sk.py [--wide-log2 16] [--log2 26] [--reps 50] [--slabs 32,512,2048]
                             [--out profiles/sk_bench.jsonl]

Times the entry points alone (device events around ``reps`` launches, the method of
tools/bench_real2complex.py) beside a device-to-device copy of the same bytes timed in the same run
(the yardstick of tools/bench_modulate.py).  Bytes moved: ``bbt_sk_excise`` reads the stream once
and writes it once -- its second read of each slab is meant to come from cache, and is not counted,
so a second read that reaches HBM shows as a lower rate --; ``bbt_sk_estimate`` reads it once
(its fraction compares bytes moved per second with the copy's, which counts the read and the write).

Shapes: (2^wide_log2, 1024, 2) complex64 with n = 256, 1024 and 4096, and (2^log2, 2) complex64
with n = 1024, each with 0 %, 10 % and 100 % of the (block, element) pairs flagged.  The data are
a constant (sk = 0, inside the limits used here) with the first sample of the flagged pairs a
thousand times stronger (sk = n, outside).  ``--slabs``: also time the wide shape at 10 % with the
tile sized for slabs of these KiB (the library's BBT_SK_SLAB_KIB, which changes no value), to see
where the second read stops finding its slab in cache.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from baseband_tasks_amd import hip                                  # noqa: E402
from bench_rows import copy_rate, timed                             # noqa: E402

LIMITS = (-0.5, 0.5)


def make(n_samples, n_elem, n, fraction, seed=1):
    """The stream in HBM and the fraction of pairs the twin's rule flags in it."""
    x = hip.DeviceArray((n_samples, n_elem), np.complex64)
    x.fill_bytes(0x3c)                                   # every float 0.0115
    n_block = n_samples // n
    base = np.frombuffer(b'\x3c' * 8, np.complex64)[0]
    rows = np.full((n_block, n_elem), base, np.complex64)
    bad = np.random.default_rng(seed).random((n_block, n_elem)) < fraction
    rows[bad] *= 1000.
    d_rows = hip.DeviceArray.from_host(rows)
    hip.copy_2d(x, n * n_elem * 8, d_rows, n_elem * 8, 0, n_elem * 8, n_block)
    hip.synchronize()
    return x, float(bad.mean())


def case(name, x, y, n, reps, copy, want_flagged, slab_kib=None):
    n_samples, n_elem = x.shape
    n_block = n_samples // n
    flags = hip.DeviceArray((n_block, n_elem), np.uint8)
    lib, st = hip.lib(), hip.get_stream()
    if slab_kib:
        os.environ['BBT_SK_SLAB_KIB'] = str(slab_kib)
    try:
        hip.sk_excise(x, y, n, n_elem, LIMITS, flags=flags)
        flagged = float(flags.to_host().mean())
        assert abs(flagged - want_flagged) < 1e-9, (flagged, want_flagged)
        t = timed(lambda: hip.check(lib.bbt_sk_excise(x.ptr, y.ptr, n_block, n, n_elem, 1, 1., LIMITS[0], LIMITS[1],
                                                      1, None, None, st)), reps)
    finally:
        os.environ.pop('BBT_SK_SLAB_KIB', None)
    sk = hip.DeviceArray((n_block, n_elem), np.float32)
    t_est = timed(lambda: hip.check(lib.bbt_sk_estimate(x.ptr, sk.ptr, n_block, n, n_elem, 1, 1., st)), reps)
    nbytes = x.nbytes
    return dict(what='sk', case=name, shape=list(x.shape), n=n, flagged=flagged, slab_kib=slab_kib or 128,
                mib=nbytes / 2**20, s_excise=t, excise_gb_per_s=2 * nbytes / t / 1e9,
                excise_copy_fraction=2 * nbytes / t / copy, s_estimate=t_est, estimate_gb_per_s=nbytes / t_est / 1e9,
                estimate_copy_fraction=nbytes / t_est / copy, copy_gb_per_s=copy / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--wide-log2', type=int, default=16)
    ap.add_argument('--log2', type=int, default=26)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--slabs', default='32,512,2048')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.set_device(0)
    copy = copy_rate((1 << args.log2) * 16, args.reps)
    lines = [json.dumps(dict(what='copy', mib=(1 << args.log2) * 16 / 2**20, gb_per_s=copy / 1e9,
                             source='hipMemcpyAsync device to device', device=hip.device_name()))]
    print(lines[0], flush=True)

    def keep(result):
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)

    slabs = [int(s) for s in args.slabs.split(',') if s]
    for name, n_samples, n_elem, ns in (('wide', 1 << args.wide_log2, 2048, (256, 1024, 4096)),
                                       ('narrow', 1 << args.log2, 2, (1024,))):
        y = hip.DeviceArray((n_samples, n_elem), np.complex64)
        for n in ns:
            for fraction in (0., 0.1, 1.):
                x, flagged = make(n_samples, n_elem, n, fraction)
                keep(case(name, x, y, n, args.reps, copy, flagged))
                if name == 'wide' and fraction == 0.1:
                    for kib in slabs:
                        keep(case(name, x, y, n, args.reps, copy, flagged, slab_kib=kib))
                del x
        del y
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
