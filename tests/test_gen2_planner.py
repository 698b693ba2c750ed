"""The generic-length engine without a GPU: what its host planner decides (csrc/gen2_host.hpp),
that the index maps of those plans give the transform (the model of tools/fft_gen2_model.py
follows every value through them and compares with numpy.fft), and that the kernel source the
library writes for a length compiles through hipRTC for gfx950 (csrc/rtc.hpp's path: the
compiler needs no device).  The lengths are the reference's default block lengths -- the
smallest 2^a 3^b 5^c 7^d >= n of its NumPy engine, baseband_tasks/fourier/numpy.py:99-126 -- and
the ones its tests use (6174: tests/test_base.py:522-529)."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('gen2') / 'gen2_plan_dump')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-I', CSRC, os.path.join(ROOT, 'tests', 'gen2_plan_dump.cpp'),
                           '-o', exe])

    def run(*args):
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True)
        return [json.loads(line) for line in out.splitlines()]
    run.exe = exe
    return run


def model():
    spec = importlib.util.spec_from_file_location('fft_gen2_model', os.path.join(ROOT, 'tools', 'fft_gen2_model.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LENGTHS = [2, 3, 14, 30, 100, 490, 540, 1000, 1536, 3000, 3087, 3402, 3430, 6174, 6561, 8100, 8192, 3125, 2401]


def test_plans_of_the_host_planner_transform_correctly(dump):
    """Every plan: the stage list multiplies to n, no stage asks a thread for more than its
    registers hold, the exchange area holds every buffer -- and the model, fed the plan's stages,
    threads and pitches, reproduces numpy.fft (forward on the plan, inverse on its reversal)."""
    m = model()
    args = []
    for n in LENGTHS:
        args += [n, 1]
    args += [490, 8, 486, 8, 30, 4]
    for pmax in (20, 12, 10):                # (row pass / column passes / channelizer: gen2_host.hpp g2_pmax)
      for plans in dump('plan', pmax, *args):
        for key, sign in (('forward', -1), ('reversed', +1)):
            g = plans[key]
            n, fac, tj = g['n'], g['fac'], g['tj']
            assert int(np.prod(fac)) == n and all(2 <= r <= min(16, pmax) for r in fac) or n == 1
            assert g['threads'] % 64 == 0 and g['threads'] >= tj * g['ct']
            ns, need = 1, 0
            for s, r in enumerate(fac):
                b = -(-(n // r) // tj)
                assert b <= 4 and b * r <= pmax, (n, fac, tj)        # (BBT_G2_MAXB, points per thread)
                assert g['slots'] >= b * r
                assert g['pitch'][s] >= ns * r
                if s + 1 < len(fac):
                    need = max(need, (n // (ns * r)) * g['pitch'][s])
                ns *= r
            assert g['lds_elems'] >= need * g['ct']
            if n <= 3500 and pmax != 12:                             # (the model is plain Python)
                m.run(n, fac=fac, sign=sign, tj=tj, pitches=g['pitch'][:len(fac) - 1], verbose=False)
        assert plans['forward']['fac'] == plans['reversed']['fac'][::-1]
        assert plans['forward']['tj'] == plans['reversed']['tj']
        assert plans['forward']['slots'] == plans['reversed']['slots']


def test_the_model_and_the_planner_agree_on_stages_and_threads(dump):
    m = model()
    for n, plans in zip(LENGTHS, dump('plan', 20, *sum(([n, 1] for n in LENGTHS), []))):
        fac = m.factorise(n)
        assert len(fac) == len(plans['forward']['fac'])
        assert m.threads(n, fac) == plans['forward']['tj'], n


def test_split_rule_prefers_workgroups_that_pack_a_cu(dump):
    """The reference's default blocks at 800 / 600 MHz and for Resample: both kernels of
    the chosen split have 1, 2, 4 or 8 waves (measured: 29.5 -> 34-35.7 Gsamples/s at 800 MHz)."""
    for n, got in zip((1666980, 3936600, 1049760, 93312), dump('split', 1666980, 3936600, 1049760, 93312)):
        assert got['n1'] * got['n2'] == n and got['n2'] <= 8192 and got['n1'] <= 1024
        for k in ('col', 'row'):
            # (blocks up to 2^17 samples: their workgroups are small, three waves pack as well)
            assert got[k]['threads'] // 64 in ((1, 2, 3, 4, 8) if n <= 2**17 else (1, 2, 4, 8)), (n, got[k])
    assert [(g['n1'], g['n2']) for g in dump('split', 1666980, 3936600, 1049760)] == [(540, 3087), (486, 8100), (240, 4374)]
    assert dump('split', 11059200) == [None]         # (N2 <= 8192 needs N1 >= 1350: the general rule takes over)


def test_short_blocks_fill_their_waves(dump):
    """Blocks of a few 10^4 samples (the defaults at low DM: 31 104 = 2^7 3^5 at 1400 MHz, DM 10) split
    into columns and rows that need a dozen threads each: a column tile takes 16 or 32 columns, a
    row workgroup up to 8 rows, so that neither kernel runs waves that are mostly idle (measured:
    Dedisperse on 31 104-sample blocks 26.7 -> 44.7 Gsamples/s), and no column is shorter than 16
    points.  Reference: the block lengths of base.py:750-758 with fourier/numpy.py:99-126."""
    got, = dump('split', 31104)
    assert (got['n1'], got['n2']) == (36, 864) and got['col']['ct'] == 32
    for n in (8232, 19200, 20000, 23328, 25725, 31104, 39366, 46656, 54432, 65610, 93312, 100000):
        g, = dump('split', n)
        assert g['n1'] * g['n2'] == n and g['n1'] >= 16
        for k in ('col', 'row'):
            fill = g[k]['tj'] * g[k]['ct'] / g[k]['threads']
            # (a 16-point column is one thread's work and a tile has at most 32 columns: half a wave)
            assert fill >= 0.5, (n, k, g[k])


def test_wide_column_tiles_of_short_blocks_are_sound(dump):
    """The plans the split rule picks for short blocks, with their 16- / 32-column tiles and several
    rows per workgroup: registers, threads and exchange area within what the kernels have, and the
    model reproduces numpy.fft on both halves.  10 080 and 10 206 are Resample's blocks on
    10 000-sample frames with pad 16 / 32 and 64 (tests/test_gpu_parity.py,
    test_random_filter_bank_channelizer_and_resampler_geometries; sampling.py:211-220 of the reference)."""
    m = model()
    for n in (8232, 10080, 10206, 19200, 20000, 31104, 46656, 65610, 93312, 100000, 129024):
        g, = dump('split', n)
        assert g is not None and g['n1'] * g['n2'] == n
        for k, pmax, lds_cap in (('col', 20, 64 * 1024), ('row', 20, 160 * 1024)):     # (BBT_G2_PMAX for both)
            p = g[k]
            fac, tj, nn = p['fac'], p['tj'], p['n']
            assert int(np.prod(fac)) == nn and all(2 <= r <= min(16, pmax) for r in fac)
            assert p['threads'] % 64 == 0 and tj * p['ct'] <= p['threads'] <= 1024
            assert p['lds_elems'] * 8 <= lds_cap, (n, k, p)
            ns, need = 1, 0
            for s, r in enumerate(fac):
                b = -(-(nn // r) // tj)
                assert b <= 4 and b * r <= pmax and p['slots'] >= b * r, (n, k, p)
                assert p['pitch'][s] >= ns * r
                if s + 1 < len(fac):
                    need = max(need, (nn // (ns * r)) * p['pitch'][s])
                ns *= r
            assert p['lds_elems'] >= need * p['ct'], (n, k, p)
            if nn <= 3500:
                m.run(nn, fac=fac, sign=-1, tj=tj, pitches=p['pitch'][:len(fac) - 1], verbose=False)


def _hiprtc():
    for name in ('libhiprtc.so.7', 'libhiprtc.so', '/opt/rocm/lib/libhiprtc.so'):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    return None


def _compile(rtc, src):
    """csrc/rtc.hpp's call of hipRTC, with the library's options; returns the code object."""
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src, b'bbt_g2.hip', 0, None, None) == 0
    opts = [b'--offload-arch=gfx950', b'-I' + CSRC.encode(), b'-O3', b'-std=c++17', b'-Wno-unused-value',
            b'-mllvm', b'-simplifycfg-sink-common=false']
    rc = rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts))
    n = C.c_size_t()
    rtc.hiprtcGetProgramLogSize(prog, C.byref(n))
    log = C.create_string_buffer(n.value + 1)
    rtc.hiprtcGetProgramLog(prog, log)
    assert rc == 0, log.value.decode(errors='replace')[-2000:]
    assert rtc.hiprtcGetCodeSize(prog, C.byref(n)) == 0 and n.value > 10000
    code = C.create_string_buffer(n.value)
    assert rtc.hiprtcGetCode(prog, code) == 0
    rtc.hiprtcDestroyProgram(C.byref(prog))
    return code.raw


def test_generated_source_compiles_through_hiprtc(dump):
    """What csrc/rtc.hpp does at plan time, without a device: source for one length -> hipRTC with
    the library's options -> a code object for gfx950 that holds both entry points."""
    rtc = _hiprtc()
    if rtc is None:
        pytest.skip('libhiprtc.so not found')
    code = _compile(rtc, subprocess.check_output([dump.exe, 'source', '6174'], text=True).encode())
    assert b'k_small' in code and b'k_rows' in code


@pytest.mark.parametrize('n', [10080, 10206, 31104])
def test_two_level_source_of_short_blocks_compiles(dump, n):
    """The translation unit of a short two-level block (row kernel with several rows per workgroup,
    column passes with 16 / 32 columns per tile), as bbt_osm_plan_create writes it: compiles for
    gfx950 with its three entry points.  10 080 / 10 206: Resample's blocks on 10000-sample frames."""
    rtc = _hiprtc()
    if rtc is None:
        pytest.skip('libhiprtc.so not found')
    src = subprocess.check_output([dump.exe, 'source2', str(n)], text=True)
    assert 'BBT_G2_KERNEL_COL(k_first' in src
    code = _compile(rtc, src.encode())
    assert b'k_row' in code and b'k_first' in code and b'k_last' in code
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    if os.path.exists(readelf):
        # (what the kernels take: no scratch memory -- nothing spilled --, exchange areas as planned)
        obj = os.path.join(os.path.dirname(dump.exe), f'g2_{n}.co')
        with open(obj, 'wb') as f:
            f.write(code)
        notes = subprocess.check_output([readelf, '--notes', obj], text=True)
        import re
        found = re.findall(r'\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+)', notes, re.S)
        assert sorted(name for _, name, _ in found) == ['k_first', 'k_last', 'k_row']
        for lds, name, scratch in found:
            assert int(scratch) == 0 and int(lds) <= 64 * 1024, (n, name, lds, scratch)


# --------------------------------------------------------------------------- the general kernels' routes
GEN_MAX_LEN, GEN_EPT, LDS_CAP = 8192, 8, 160 * 1024      # (csrc/gen_geo.hpp; LDS of a CU of gfx950)
MODES = ('off', 'on', 'failed')


def smooth_lengths(lo, hi):
    """Every 2^a 3^b 5^c 7^d in (lo, hi], ascending."""
    out = []
    p7 = 1
    while p7 <= hi:
        p5 = p7
        while p5 <= hi:
            p3 = p5
            while p3 <= hi:
                p2 = p3
                while p2 <= hi:
                    if p2 > lo:
                        out.append(p2)
                    p2 *= 2
                p3 *= 3
            p5 *= 5
        p7 *= 7
    return sorted(out)


def _package_module(name):
    """A module of the package without the package's own import (which loads the library)."""
    import types
    pkg = 'bbt_planner_pkg'
    if pkg not in sys.modules:
        stub = types.ModuleType(pkg)
        stub.__path__ = [os.path.join(ROOT, 'baseband-tasks_amd')]
        sys.modules[pkg] = stub
    return importlib.import_module(f'{pkg}.{name}')


def route_faults(g):
    """What of the general kernels' contract (csrc/fft_generic.hpp: a tile of n * ct <= BBT_GEN_MAX_LEN
    elements, every stage of radix R covering it with ceil(BBT_GEN_EPT / R) butterflies per thread)
    the route `g` of one block length breaks: a list of words, empty if it is sound."""
    bad = []
    n, n1, n2, ct = g['n'], g['n1'], g['n2'], g['ct']
    if n1 * n2 != n or int(np.prod(g['fac1'])) != n1 or int(np.prod(g['fac2'])) != n2:
        bad.append('product')
    if n2 > GEN_MAX_LEN:
        bad.append('n2')
    if ct < 1 or ct & (ct - 1) or g['col_threads'] % ct:
        bad.append('ct')
    if n1 * ct > GEN_MAX_LEN:
        bad.append('tile')
    if g['col_lds'] != n1 * ct * 16 or g['row_lds'] != n2 * 16 or max(g['col_lds'], g['row_lds']) > LDS_CAP:
        bad.append('lds')
    for fac, threads, elems in ((g['fac1'], g['col_threads'], n1 * ct), (g['fac2'], g['row_threads'], n2)):
        if threads % 64 or not 64 <= threads <= 1024:
            bad.append('threads')
        if any(r * -(-GEN_EPT // r) * threads < elems for r in fac):
            bad.append('stage')
    return bad


def test_every_block_length_gets_a_sound_route_on_the_general_kernels(dump):
    """Every block length the Python side hands the library (fourier.py: HipFFTMaker._transformable,
    2^a 3^b 5^c 7^d in (8192, 2^26] that are not powers of two), in every mode of plan-time compilation -- off
    (BBT_RTC=0), on, and on but failed, when the general kernels run with the split and the tile chosen
    for the compiled ones: N1 x N2 = N, N2 <= 8192, a tile of `ct` columns (a power of two that
    divides the workgroup) within BBT_GEN_MAX_LEN elements and 160 KiB of LDS, and every stage
    of both factors reaching the whole tile (`R * ceil(BBT_GEN_EPT / R) * threads >= elements`,
    the caller's contract of fft_generic.hpp).  A tile beyond that is transformed in part, without
    an error."""
    fourier = _package_module('fourier')
    lengths = [n for n in smooth_lengths(8192, 2**26) if n & (n - 1) and fourier.HipFFTMaker._transformable(n)]
    assert len(lengths) == 2792
    for mode in MODES:
        routes = dump('route', mode, *lengths)
        assert None not in routes, (mode, [n for n, g in zip(lengths, routes) if g is None][:10])
        faults = [(g['n'], g['n1'], g['n2'], g['ct'], route_faults(g)) for g in routes if route_faults(g)]
        assert not faults, (mode, len(faults), faults[:8])
        assert [g['n'] for g in routes] == lengths


def test_python_and_c_agree_on_the_lengths_that_split(dump):
    """`HipFFTMaker._transformable` (fourier.py) and `_splits` (conversion.py) accept a block length
    exactly when the library's split rule finds two factors for it: every 2^a 3^b 5^c 7^d in
    (8192, 2^26], powers of two included, with plan-time compilation on and off."""
    fourier, conversion = _package_module('fourier'), _package_module('conversion')
    lengths = smooth_lengths(8192, 2**26)
    assert len(lengths) + len(smooth_lengths(0, 8192)) == 3174          # (the count fourier.py states)
    splits = [conversion._splits(n) for n in lengths]
    transformable = [fourier.HipFFTMaker._transformable(n) for n in lengths]
    for mode in ('off', 'on'):
        routes = dump('route', mode, *lengths)
        assert len(routes) == len(lengths)
        for n, g, s, t in zip(lengths, routes, splits, transformable):
            assert (g is not None) == s, (mode, n)
            if n & (n - 1):              # (powers of two: their own plans, up to 2^24)
                assert (g is not None) == t, (mode, n)
    refused = [n for n, t in zip(lengths, transformable) if not t]
    assert len(refused) == 52 and refused[0] == 20588575        # (5^2 7^7: fourier.py)
