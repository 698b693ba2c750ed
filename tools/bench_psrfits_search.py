"""Rates of the PSRFITS search-mode coding, one JSON line per case (dev tool).

    python tools/bench_psrfits_search.py [--rows 8] [--shape 4096,1024,4] [--bits 8,4,2,1] [--file-bits 8,2]
                                         [--file-rows 4] [--reps 20] [--dir /tmp]
                                         [--out profiles/psrfits_search_bench.jsonl]

Kernels, HBM-resident: bbt_psrsearch_encode and bbt_psrsearch_decode on ``--rows`` rows of ``--shape``
(nsblk, channels, polarizations) float32 at every width of ``--bits``, each timed with device events
after a warm-up call (the method of tools/bench_real2complex.py).  Reported: bytes moved per second,
4 read and nbits / 8 written per sample for the encoder (its second read of a slab, meant to come
from L2, is not counted) and the reverse for the decoder, beside a device-to-device copy of the
input's size in the same run.

Files: the waterfall ``Integrate(Power(Channelize(noise, nchan)), 4)`` of ``--rows`` rows streamed
into a file under ``--dir`` two ways (wall time, best of three, the file closed inside the timed
region): ``device_pieces``, ``stream.read(out=writer)`` -- the rows are coded in HBM and bytes,
scales, offsets and counts come down --; and ``host_route``, ``stream.read()`` to the host, then
`psrfits.encode_search_rows` and the same writer.  The waterfall itself (the same in both) is timed
alone as ``read_device``.
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


def kernels(x, rows, dims, nbits, reps, copy):
    nsblk, n_chan, n_pol = dims
    lib = hip.lib()
    nsigma = psrfits.SEARCH_NSIGMA[nbits]
    codes, scl, offs, n_finite = hip.psrsearch_encode(x, nsblk, nbits, nsigma)
    out = hip.DeviceArray(x.shape, np.float32)
    moved = x.size * 4 + codes.size

    def encode():
        hip.check(lib.bbt_psrsearch_encode(x.ptr, codes.ptr, scl.ptr, offs.ptr, n_finite.ptr, rows, nsblk, n_chan,
                                           n_pol, nbits, nsigma, hip.get_stream()))

    for what, fn in (('psrsearch_encode', encode),
                     ('psrsearch_decode', lambda: hip.psrsearch_decode(codes, scl, offs, None, 0., nbits, dims, out=out))):
        t = timed(fn, reps)
        yield dict(what=what, nbits=nbits, rows=rows, nsblk=nsblk, n_chan=n_chan, n_pol=n_pol,
                   float_mib=x.nbytes / 2**20, s_per_call=t, gb_per_s=moved / t / 1e9, copy_gb_per_s=copy / 1e9,
                   copy_fraction=moved / t / copy)


def files(rows, dims, nbits, where):
    nsblk, n_chan, n_pol = dims
    if n_pol != 4:
        raise SystemExit("the file cases write Power (4 polarizations) of a channelized stream")
    n = rows * nsblk * 4 * n_chan
    t0 = bt.Time('2020-01-01T00:00:00')
    noise = bt.DeviceNoiseGenerator((n, 2), t0, 16 * u.MHz, 1 << 20, seed=2, frequency=1400 * u.MHz, sideband=1,
                                    polarization=['X', 'Y'])
    stream = bt.Integrate(bt.Power(bt.Channelize(noise, n_chan)), 4, samples_per_frame=nsblk)
    stream.read_device(nsblk)                           # (plans made, buffers allocated)
    hip.synchronize()
    keys = dict(template=stream, nbits=nbits, nsblk=nsblk)

    def device_pieces(path):
        with psrfits.open_search(path, 'w', **keys) as fw:
            stream.read(out=fw)

    def host_route(path):
        spectrum = stream.read()
        with psrfits.open_search(path, 'w', **keys) as fw:
            fw.write(spectrum)

    def read_only(path):
        for _ in range(rows):
            stream.read_device(nsblk)
        hip.synchronize()

    for name, run in (('read_device', read_only), ('device_pieces', device_pieces), ('host_route', host_route)):
        path = os.path.join(where, f'bench_psrfits_search_{name}.fits')
        best = None
        for _ in range(3):
            stream.seek(0)
            stream.invalidate_cache()
            t_start = time.perf_counter()
            run(path)
            t = time.perf_counter() - t_start
            best = t if best is None else min(best, t)
        size = os.path.getsize(path) if os.path.exists(path) else 0
        if size:
            os.remove(path)
        yield dict(what='waterfall_to_file', route=name, nbits=nbits, rows=rows, nsblk=nsblk, n_chan=n_chan,
                   n_pol=n_pol, file_mib=size / 2**20, s_best_of_3=best,
                   float_gb_per_s=stream.shape[0] * n_chan * n_pol * 4 / best / 1e9, directory=where)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=8)
    ap.add_argument('--shape', default='4096,1024,4')
    ap.add_argument('--bits', default='8,4,2,1')
    ap.add_argument('--file-bits', default='8,2')
    ap.add_argument('--file-rows', type=int, default=4)
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

    def keep(result):
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(1)
    x = hip.DeviceArray.from_host(
        (rng.standard_normal((args.rows * dims[0],) + dims[1:] + (2,), dtype=np.float32) ** 2).sum(-1))
    for nbits in (int(b) for b in args.bits.split(',')):
        for result in kernels(x, args.rows, dims, nbits, args.reps, copy):
            keep(result)
    del x
    for nbits in (int(b) for b in args.file_bits.split(',')):
        by = {}
        for result in files(args.file_rows, dims, nbits, args.dir):
            by[result['route']] = result['s_best_of_3']
            keep(result)
        keep(dict(what='ratio', nbits=nbits, host_route_over_device_pieces=by['host_route'] / by['device_pieces']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
