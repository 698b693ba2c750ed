"""Rates of the PSRFITS fold-mode coding, one JSON line per case (dev tool).

    python tools/bench_psrfits.py [--rows 4] [--shape 1024,4096,4] [--reps 20] [--dir /tmp]
                                  [--out profiles/psrfits_bench.jsonl]

Kernels, HBM-resident: bbt_psrfits_encode and bbt_psrfits_decode on ``--rows`` rows of ``--shape``
(bins, channels, polarizations) float32, each timed with device events after a warm-up call (the
method of tools/bench_real2complex.py).  Reported: bytes moved per second, 4 read and 2 written per
sample for the encoder (its second read of a slab, meant to come from L2, is not counted) and the
reverse for the decoder, beside a device-to-device copy of the input's size in the same run.

Files: a `Fold` of ``--rows`` profiles of that shape streamed into an archive under ``--dir`` two
ways (wall time, best of three, the file closed inside the timed region): ``device_pieces``,
``fold.read(out=writer)`` -- the profiles are coded in HBM and codes, scales, offsets and counts
come down --; and ``host_route``, the only route before the writer existed: ``fold.read()`` to the
host, then `psrfits.encode_rows` and the same writer.  The fold itself (the same in both) is timed
alone as ``fold_read_device``.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baseband_tasks_amd as bt                                     # noqa: E402
from baseband_tasks_amd import hip, psrfits                         # noqa: E402
from baseband_tasks_amd import units as u                           # noqa: E402
from bench_rows import copy_rate, timed                             # noqa: E402


def kernels(rows, dims, reps, copy):
    n_bin, n_chan, n_pol = dims
    rng = np.random.default_rng(1)
    x = hip.DeviceArray.from_host(rng.standard_normal((rows, n_bin, n_chan, n_pol)).astype(np.float32))
    lib = hip.lib()
    codes, scl, offs, n_finite = hip.psrfits_encode(x)
    out = hip.DeviceArray(x.shape, np.float32)
    moved = x.size * 6

    def encode():
        hip.check(lib.bbt_psrfits_encode(x.ptr, codes.ptr, scl.ptr, offs.ptr, n_finite.ptr, rows, n_bin, n_chan,
                                         n_pol, hip.get_stream()))

    for what, fn in (('psrfits_encode', encode),
                     ('psrfits_decode', lambda: hip.psrfits_decode(codes, scl, offs, out=out))):
        t = timed(fn, reps)
        yield dict(what=what, rows=rows, n_bin=n_bin, n_chan=n_chan, n_pol=n_pol, float_mib=x.nbytes / 2**20,
                   s_per_call=t, gb_per_s=moved / t / 1e9, copy_gb_per_s=copy / 1e9, copy_fraction=moved / t / copy)


def files(rows, dims, where):
    n_bin, n_chan, n_pol = dims
    if n_pol not in (1, 4):
        raise SystemExit("the file cases fold Square (1 polarization) or Power (4) of a channelized stream")
    per_row = 4 * n_bin                                 # spectra per profile: a few per bin
    n = rows * per_row * n_chan
    rng = np.random.default_rng(2)
    streams = 2 if n_pol == 4 else 1
    z = rng.standard_normal((n, streams, 2)).astype(np.float32).view(np.complex64)[..., 0]
    t0 = bt.Time('2020-01-01T00:00:00')
    keys = dict(frequency=1400 * u.MHz, sideband=1)
    if n_pol == 4:
        keys['polarization'] = ['X', 'Y']
    ds = bt.DeviceStream(z, t0, 16 * u.MHz, **keys)
    ch = bt.Channelize(ds, n_chan)
    detected = bt.Power(ch) if n_pol == 4 else bt.Square(ch)
    f0 = 16e6 / n_chan / (n_bin * 1.37)                 # (a period of 1.37 bins' worth of spectra per bin)
    fold = bt.Fold(detected, n_bin, lambda t: f0 * (t - t0), step=per_row)
    fold.read_device(1)                                 # (plans made, buffers allocated)
    hip.synchronize()

    def device_pieces(path):
        with psrfits.open(path, 'w', template=fold) as fw:
            fold.read(out=fw)

    def host_route(path):
        profiles = fold.read()
        with psrfits.open(path, 'w', template=fold) as fw:
            fw.write(profiles)

    def fold_only(path):
        for _ in range(fold.shape[0]):
            fold.read_device(1)
        hip.synchronize()

    for name, run in (('fold_read_device', fold_only), ('device_pieces', device_pieces), ('host_route', host_route)):
        path = os.path.join(where, f'bench_psrfits_{name}.fits')
        best = None
        for _ in range(3):
            fold.seek(0)
            fold.invalidate_cache()
            t_start = time.perf_counter()
            run(path)
            t = time.perf_counter() - t_start
            best = t if best is None else min(best, t)
        size = os.path.getsize(path) if os.path.exists(path) else 0
        if size:
            os.remove(path)
        yield dict(what='fold_to_archive', route=name, rows=rows, n_bin=n_bin, n_chan=n_chan, n_pol=n_pol,
                   file_mib=size / 2**20, s_best_of_3=best, profile_gb_per_s=fold.size * 4 / best / 1e9,
                   directory=where)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4)
    ap.add_argument('--shape', default='1024,4096,4')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--dir', default=tempfile.gettempdir())
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dims = tuple(int(d) for d in args.shape.split(','))
    assert len(dims) == 3
    hip.set_device(0)
    nbytes = args.rows * dims[0] * dims[1] * dims[2] * 4
    copy = copy_rate(nbytes, args.reps)
    lines = [json.dumps(dict(what='copy', mib=nbytes / 2**20, gb_per_s=copy / 1e9,
                             source='hipMemcpyAsync device to device'))]
    print(lines[0], flush=True)
    for result in list(kernels(args.rows, dims, args.reps, copy)) + list(files(args.rows, dims, args.dir)):
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)
    by = {r['route']: r['s_best_of_3'] for r in map(json.loads, lines) if r['what'] == 'fold_to_archive'}
    lines.append(json.dumps(dict(what='ratio', host_route_over_device_pieces=by['host_route'] / by['device_pieces'])))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
