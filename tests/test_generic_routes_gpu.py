"""Block lengths that are not powers of two on every route the library has for them, against the
float64 oracle: the kernels compiled for the length when the plan is made (csrc/fft_gen2.hpp), and
the general LDS Stockham kernels (csrc/fft_generic.hpp, gen_kernels.hpp: k_gen_col, k_gen_row,
k_gen_osm_small, k_gen_fft_rows, k_r2c_gen) that take over when compilation is switched off or
fails.  The environment decides the route, so every mode runs in a child process of its own:

  a  default: plan-time compilation on
  b  BBT_RTC=0: the general kernels, with their own split and 8-column tiles
  c  compilation on but failing (BBT_CSRC points nowhere): the general kernels with the split and
     the 16- / 32-column tiles chosen for the compiled ones, after one warning
  d  no hipRTC in the process (BBT_HIPRTC_LIB points nowhere, BBT_HIPRTC_ONLY=1): as c

The child asserts the mode it runs in and every figure (after printing it); the parent asserts
the return code, that nothing was compiled on the fall-back routes and that the 'general kernels'
warning was printed once when compilation failed.

Contract: `assert_parity` of tests/test_gpu_parity.py -- relative L2 <= 1e-6 and max <= 1e-5 rms
against the float64 oracle.  The lengths, with split N1 x N2 and columns per tile of
the general kernels as tests/gen2_plan_dump.cpp `route` prints them (b | c; the compiled kernels
take c's split and tile):

  8232       84 x 98, 8     | 42 x 196, 32       short blocks whose compiled plan takes 32 ...
  31104      162 x 192, 8   | 36 x 864, 32
  10080      96 x 105, 8    | 42 x 240, 32
  10206      81 x 126, 8    | 81 x 126, 16       ... and 16 columns
  8505       81 x 105, 8    | 81 x 105, 16       (N1 = 81)
  1666980    490 x 3402, 8  | 540 x 3087, 8      a long block after a failed compilation
  2941225    1715 x 1715, 4 | the same           the first length of the older split rule (before the
                                                 tile rule was mended: 8 columns, 214 KiB of LDS asked)
  3828125    1225 x 3125, 4 | 625 x 6125, 8      radices 7 and 5 only (before: 8 columns, 9800 elements
                                                 in a tile of 8192; every stage reaches 10 240)
  10485760   2560 x 4096, 2 | the same           radices 8, 8, 8, 5 (before: 4 columns, 10 240
                                                 elements of which the radix-8 stages reach 8192)
  11059200   3200 x 3456, 2 | the same           no split by the measured rule (test_gen2_planner.py)
  16941456   4116 x 4116, 1 | the same           N1 > 4096: one column per tile
  33592320   5760 x 5832, 1 | the same           the smallest such length above 2^25

The last one's float64 oracle (three blocks, two streams) takes 13 s on the host of an MI355X.

Measured on an MI355X: relative L2 2.8e-7 ... 4.1e-7 for the short blocks in every mode, 3.4e-7 ...
5.7e-7 for the long ones (the largest, 10 485 760 on the compiled kernels), max / rms at most
3.5e-6.  The library before the tile rule was mended, with BBT_RTC=0: 2 941 225 and 3 828 125 an
error (the tile's LDS), 10 485 760 a relative L2 of 5.07 without one."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from oracle import bbt_oracle as orc
from conftest import rel_l2, max_over_rms
from test_gpu_parity import REL_L2_TOL, MAX_TOL
from test_conversion_gpu import check as r2c_check, reference as r2c_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = '2020-01-01T00:00:00'
MODES = {'a': dict(BBT_RTC='1'),
         'b': dict(BBT_RTC='0'),
         'c': dict(BBT_RTC='1', BBT_CSRC=os.path.join(ROOT, 'tests', 'no-such-directory')),
         'd': dict(BBT_RTC='1', BBT_HIPRTC_LIB=os.path.join(ROOT, 'tests', 'no-such-libhiprtc.so'), BBT_HIPRTC_ONLY='1')}
RTC_MODE = {'a': 'on', 'b': 'off', 'c': 'on', 'd': 'on'}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not bt.hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


# --------------------------------------------------------------------------- shared by parent and child
def convolve_inputs(n_fft, n_stream):
    """Seeded complex noise on `n_stream` streams, two and a half blocks and a few samples (a short
    last block is read), and a random complex response of min(n_fft // 3, 40000) taps per stream."""
    n_tap = max(2, min(n_fft // 3, 40000))
    rng = np.random.default_rng(n_fft + n_stream)
    resp = ((rng.standard_normal((n_tap, n_stream)) + 1j * rng.standard_normal((n_tap, n_stream)))
            / np.sqrt(n_tap)).astype(np.complex64)
    n_in = 2 * n_fft + n_fft // 2 + 5
    x = rng.standard_normal((n_in, 2 * n_stream), dtype=np.float32).view(np.complex64)
    return x, resp, n_tap


def convolve_oracle(x, resp, n_fft, n_tap):
    want, info = orc.convolve(x, resp, samples_per_frame=n_fft - n_tap + 1, ih_samples_per_frame=1000)
    assert info['ih_spf'] == n_fft
    return want


def report(what, got, want):
    """Print the figures, then hold them to the contract of tests/test_gpu_parity.py."""
    assert got.shape == want.shape and got.dtype == np.complex64, (what, got.shape, want.shape, got.dtype)
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    print(f'CASE {what}: rel-L2 {e2:.3e} max/rms {em:.3e}', flush=True)
    return e2 <= REL_L2_TOL and em <= MAX_TOL


def child(arg):
    """What a child process runs: `arg` is JSON, dict(mode=..., kind=..., cases=[...])."""
    job = json.loads(arg)
    assert bt.hip.rtc_info()['mode'] == RTC_MODE[job['mode']]
    bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0           # the Fourier-domain plan, not the direct FIR
    ok = True
    if job['kind'] == 'convolve':
        for n_fft, n_stream, want_file in job['cases']:
            x, resp, n_tap = convolve_inputs(n_fft, n_stream)
            cv = bt.Convolve(bt.DeviceStream(x, T0, 1 * u.MHz), resp, samples_per_frame=n_fft - n_tap + 1)
            assert cv._ih_samples_per_frame == n_fft
            got = cv.read()
            del cv
            want = np.load(want_file) if want_file else convolve_oracle(x, resp, n_fft, n_tap)
            ok = report(f'convolve n_fft {n_fft} streams {n_stream} mode {job["mode"]}', got, want) and ok
            del x, got, want
    elif job['kind'] == 'r2c':
        for m, shape, frames in job['cases']:
            x = np.random.default_rng(m + frames).standard_normal((2 * m * frames,) + tuple(shape)).astype(np.float32)
            r2c = bt.Real2Complex(bt.DeviceStream(x, T0, 64 * u.kHz, samples_per_frame=2 * m))
            assert r2c.one_pass
            out = r2c.read()
            print(f'CASE r2c m {m} shape {tuple(shape)} frames {frames} mode {job["mode"]}: rel-L2 '
                  f'{rel_l2(out, r2c_reference(x, m)):.3e}', flush=True)
            r2c_check(out, x, m)
    elif job['kind'] == 'channelize':
        for n, n_stream in job['cases']:
            x = np.random.default_rng(n).standard_normal((37 * n, 2 * n_stream), dtype=np.float32).view(np.complex64)
            z = bt.Channelize(bt.DeviceStream(x, T0, 1 * u.MHz), n).read()
            ok = report(f'channelize {n} streams {n_stream} mode {job["mode"]}', z, orc.channelize(x, n)) and ok
            back = bt.Dechannelize(bt.DeviceStream(z, T0, 1 * u.MHz / n), n).read()
            ok = report(f'dechannelize {n} streams {n_stream} mode {job["mode"]}', back, x) and ok
    else:
        raise ValueError(job['kind'])
    print('INFO modules %d' % bt.hip.rtc_info()['modules'], flush=True)
    assert ok, 'a case above misses relative L2 <= 1e-6 or max <= 1e-5 rms'


def run_child(mode, kind, cases, timeout=280, compiles=True):
    """One child process in `mode`; returns its output.  `compiles`: whether these cases ask for
    plan-time compilation at all (every case of this file does: only then is there a warning)."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_generic_routes_gpu as t; t.child(sys.argv[1])"
            % (ROOT, os.path.join(ROOT, 'tests')))
    env = dict(os.environ, **MODES[mode])
    if mode == 'a':
        env.pop('BBT_CSRC', None)
    out = subprocess.run([sys.executable, '-c', code, json.dumps(dict(mode=mode, kind=kind, cases=cases))],
                         env=env, capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.count('CASE ') >= len(cases)
    modules = int(out.stdout.split('INFO modules')[-1].split()[0])
    if mode == 'a':
        assert modules >= 1, out.stdout
    else:
        assert modules == 0, out.stdout
    if mode in 'cd' and compiles:
        # (the warning names the general kernels, once per process)
        assert out.stderr.count('general kernels') == 1, out.stderr[-3000:]
    return out.stdout


def started_in_another_mode(mode):
    """A process started with BBT_RTC=0 (or `require`) asks for that everywhere: the modes that
    need compilation on cannot be set up under it."""
    if os.environ.get('BBT_RTC', '1') not in ('', '1') and mode == 'a':
        pytest.skip('BBT_RTC is set in the environment: the default mode is not what runs')


# --------------------------------------------------------------------------- short two-level blocks
@pytest.mark.parametrize('mode', ['a', 'b', 'c'])
@pytest.mark.parametrize('n_fft', [8232, 31104, 10080, 10206, 8505])
def test_short_blocks_with_wide_column_tiles(n_fft, mode):
    """Two-level blocks up to 2^17 samples: the compiled plan takes 32 (8232 = 42 x 196, 31 104 =
    36 x 864, 10 080 = 42 x 240) or 16 columns per tile (10 206 = 81 x 126, 8505 = 81 x 105), and
    after a failed compilation k_gen_col runs with those tiles (mode c); with compilation off (b) it
    takes 8 columns of another split.  2 and 6 streams."""
    started_in_another_mode(mode)
    run_child(mode, 'convolve', [[n_fft, 2, None], [n_fft, 6, None]])


@pytest.mark.parametrize('n_fft', [8232, 10206])
def test_short_blocks_without_hiprtc_in_the_process(n_fft):
    """Mode d for a 32- and a 16-column tile: the loader finds no hipRTC, the general kernels run."""
    run_child('d', 'convolve', [[n_fft, 2, None], [n_fft, 6, None]])


# --------------------------------------------------------------------------- long blocks
LONG = [(1666980, 'c'), (2941225, 'abc'), (3828125, 'abc'), (10485760, 'abc'), (11059200, 'abc'), (16941456, 'abc'),
        (33592320, 'abc')]


@pytest.mark.parametrize('n_fft, modes', LONG, ids=[str(n) for n, _ in LONG])
def test_long_blocks_on_every_route(n_fft, modes, tmp_path):
    """Blocks of 1.7 M to 33.6 M samples on two streams (module docstring: split, tile and what
    each length is there for), one child per mode against one float64 oracle, which the parent
    computes once and hands over in a file.  Mode d: 2 941 225 only."""
    x, resp, n_tap = convolve_inputs(n_fft, 2)
    t0 = time.time()
    want = convolve_oracle(x, resp, n_fft, n_tap)
    print(f'n_fft {n_fft}: float64 oracle {time.time() - t0:.1f} s on the host')
    want_file = str(tmp_path / 'want.npy')
    np.save(want_file, want)
    del x, want
    try:
        for mode in modes + ('d' if n_fft == 2941225 else ''):
            if mode == 'a' and os.environ.get('BBT_RTC', '1') not in ('', '1'):
                continue
            run_child(mode, 'convolve', [[n_fft, 2, want_file]], timeout=600)
    finally:
        os.unlink(want_file)


def test_dedisperse_default_block_above_the_older_split_rule():
    """`Dedisperse` with default arguments at 16 MHz around 1000 MHz and DM 400: four times the
    padding asks for a block of 3 402 000 = 1800 x 1890 samples, past the length (2 941 225) from
    which the measured split rule can give out -- the chirp made on the GPU (bbt_chirp) at such a
    length, against orc.dedisperse."""
    n_in = 2 * 3402000 + 3402000 // 2 + 5
    nh = bt.NoiseGenerator((n_in, 2), T0, 16 * u.MHz, 2**16, seed=400, frequency=1000 * u.MHz, sideband=1)
    dd = bt.Dedisperse(nh, 400.)
    print('Dedisperse(DM 400): block', dd._ih_samples_per_frame, 'padding', dd._pad_start, dd._pad_end)
    x = orc.noise_stream(400, 0, n_in, 2**16, (2,))
    want, info = orc.dedisperse(x, 16e6, 1000., 1, 400., ih_samples_per_frame=2**16,
                                fast_len=bt.fourier.HipFFTMaker.next_fast_len)
    assert dd._ih_samples_per_frame == info['ih_spf'] == 3402000 > 2941225
    got = dd.read()
    assert report('dedisperse block 3402000', got, want)


# --------------------------------------------------------------------------- Real2Complex
@pytest.mark.parametrize('mode', ['b', 'c'])
def test_real2complex_on_the_general_kernel(mode):
    """k_r2c_gen (every one-pass length when nothing can be compiled, powers of two included):
    output frames of 6, 1000, 1024, 6174 and 8192 samples, sample shapes (), (2,), (3,), (8,) -- the
    three access widths: one float, pairs, four streams at a time -- and 1 ... 5 frames, against
    `check` of tests/test_conversion_gpu.py (float64 restatement of the reference, relative L2 <=
    2e-6, real part equal to the even input samples bit for bit)."""
    cases = [[m, list(shape), 1 + (i + j) % 5]
             for i, m in enumerate((6, 1000, 1024, 6174, 8192)) for j, shape in enumerate(((), (2,), (3,), (8,)))]
    cases += [[1000, [2], frames] for frames in (1, 2, 3, 4, 5)] + [[6174, [], frames] for frames in (1, 2, 4, 5)]
    run_child(mode, 'r2c', cases)


# --------------------------------------------------------------------------- Channelize / Dechannelize
def test_channelizer_after_a_failed_compilation():
    """k_gen_fft_rows in mode c (mode b: test_general_and_specialised_kernels_agree_with_the_oracle):
    1000, 6174 and 360 channels on 2 and 16 streams, there and back."""
    run_child('c', 'channelize', [[n, s] for n in (1000, 6174, 360) for s in (2, 16)])
