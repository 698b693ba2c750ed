"""`Correlate` on the GPU, held to its rule: exact on integer data, within the derived bound of
`correlate_samples` on Gaussian data, bit for bit the same whatever the budget, the framing, the reads
or the tiling, equal to `Integrate(Power)` for two inputs, and in a chain from three stacked streams to an
HDF5 file.

Largest measured ratio of error to bound on the Gaussian cases (MI355X): 0.42 (33 inputs, n = 3), 0.006 to
0.018 from n = 1023 on, 0.08 in the chain."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hdf5

import corr_cases
from corr_cases import BY_NAME, IDS, same_bits, set_tiling

pytestmark = pytest.mark.gpu


def _device(x, **kwargs):
    return corr_cases.stream(x, bt.DeviceStream, **kwargs)


def _autos(case):
    """The index of the autocorrelations along the baseline axis."""
    pairs = bt.baseline_pairs(corr_cases.n_inputs(case))
    return np.flatnonzero(pairs[:, 0] == pairs[:, 1])


@pytest.mark.parametrize('name', IDS)
def test_exact_on_integer_data(name, monkeypatch):
    """Integer parts in [-7, 7]: every partial sum is an integer below 2^24, so every order of addition is
    exact, the sums come out bit for bit and the averages as float32(total / n) from float64."""
    set_tiling(monkeypatch)
    case = BY_NAME[name]
    x = corr_cases.integer_data(name)
    ax = 1 + case.axis % len(case.sample_shape)
    for average in (False, True):
        task = bt.Correlate(_device(x), case.n, case.axis, average=average)
        assert task.shape == (case.blocks,) + bt.correlate_samples(x[:case.n], case.n, case.axis).shape[1:]
        got = task.read()
        want = corr_cases.integer_expected(name, average)
        assert got.dtype == np.complex64 and same_bits(got, want), (name, average, np.argwhere(got != want)[:5])
        autos = np.take(got, _autos(case), axis=ax)
        assert not np.ascontiguousarray(autos.imag).view(np.uint32).any()          # +0, not -0
        task.close()


@pytest.mark.parametrize('name', IDS)
def test_gaussian_within_the_bound(name, monkeypatch):
    """|got - want| <= (min(n, SEG) + 4) 2^-24 S per part against the float64 values: K u sum |a b| of a K-term fma
    chain, plus the combining operation, the float64 sums and the roundings at the end."""
    set_tiling(monkeypatch)
    case = BY_NAME[name]
    x = corr_cases.gaussian_data(name)
    for average in (True, False):
        task = bt.Correlate(_device(x), case.n, case.axis, average=average)
        got = task.read()
        want = bt.correlate_samples(x, case.n, case.axis, average=average)
        ratio = corr_cases.within_bound(got, want, x, case, average)
        print(f'corr error/bound {name} average={average}: {ratio:.4f}')
        assert got.shape == want.shape and ratio <= 1., (name, average, ratio)
        ax = 1 + case.axis % len(case.sample_shape)
        assert not np.ascontiguousarray(np.take(got, _autos(case), axis=ax).imag).view(np.uint32).any()
        task.close()


def _read(x, case, budget=None, spf=1, monkeypatch=None, tiling=(None, None), how='whole'):
    set_tiling(monkeypatch, *tiling)
    task = bt.Correlate(_device(x), case.n, case.axis, samples_per_frame=spf)
    if budget is not None:
        task.correlate_budget = budget
    if how == 'whole':
        out = task.read()
    elif how == 'two':
        out = np.concatenate([task.read(1), task.read()])
    else:
        task.seek(1)
        out = task.read()
    task.close()
    return out


@pytest.mark.parametrize('name', corr_cases.INDEPENDENCE)
def test_independent_of_the_cutting(name, monkeypatch):
    """Device against device, bit for bit: the budget (a segment per fetch; a block per fetch; two blocks per
    fetch; the default), the framing, a read in two pieces, a seek, and every tiling the geometry accepts."""
    case = BY_NAME[name]
    x = corr_cases.gaussian_data(name)
    row = int(np.prod(case.sample_shape)) * 8
    base = _read(x, case, monkeypatch=monkeypatch)
    assert base.shape[0] == case.blocks == 2 and np.isfinite(base.view(np.float32)).all() and base.any()
    budgets = (corr_cases.SEG * row, 2 * corr_cases.SEG * row, case.n * row, 2 * case.n * row, 1)
    for budget in budgets:
        for spf in (1, 3):
            assert same_bits(_read(x, case, budget, spf, monkeypatch), base), (name, budget, spf)
    task = bt.Correlate(_device(x), case.n, case.axis)
    task.correlate_budget = corr_cases.SEG * row
    assert task._piece_size() == corr_cases.SEG and task._input_span(0, 1) is None        # several fetches per block
    task.correlate_budget = 2 * case.n * row
    assert task._piece_size() == 2 * case.n and task._input_span(0, 2)[1:] == (0, 2 * case.n)
    task.close()
    assert same_bits(_read(x, case, corr_cases.SEG * row, 1, monkeypatch, how='two'), base)
    assert same_bits(_read(x, case, None, 1, monkeypatch, how='two'), base)
    assert same_bits(_read(x, case, corr_cases.SEG * row, 1, monkeypatch, how='seek'), base[1:])
    assert same_bits(_read(x, case, None, 3, monkeypatch, how='seek'), base[1:])
    for tiling in corr_cases.tilings(corr_cases.n_inputs(case)):
        assert same_bits(_read(x, case, None, 1, monkeypatch, tiling), base), (name, tiling)
        assert same_bits(_read(x, case, corr_cases.SEG * row, 1, monkeypatch, tiling), base), (name, tiling)


def test_read_device_leaves_the_visibilities_in_hbm(monkeypatch):
    set_tiling(monkeypatch)
    name = 'a5-e7-n1023-b2-t1'
    case, x = BY_NAME[name], corr_cases.integer_data(name)
    task = bt.Correlate(_device(x), case.n)
    got = task.read_device()
    assert isinstance(got, bt.hip.DeviceArray) and got.dtype == np.complex64
    assert same_bits(got.to_host(), corr_cases.integer_expected(name, True))
    task.close()


@pytest.mark.parametrize('average', [False, True], ids=['sums', 'averages'])
def test_two_inputs_equal_integrate_power(average, monkeypatch):
    """On integer data rows 0, 2 and 1 (real and imaginary) are XX, YY and Re, Im of XY of `Power`, integrated."""
    set_tiling(monkeypatch)
    name = 'a2-e40-n1024-b3-t5'
    case, x = BY_NAME[name], corr_cases.integer_data(name)
    pol = np.array(['X', 'Y'])
    got = bt.Correlate(_device(x, polarization=pol), case.n, average=average).read()
    power = bt.Integrate(bt.Power(_device(x, polarization=pol)), case.n, average=average).read()
    if not average:
        assert (power['count'] == case.n).all()               # (sums come from Integrate with their counts)
        power = power['data']
    assert power.shape == (3, 40, 4) and got.shape == (3, 40, 3)
    assert same_bits(got[..., 0].real, power[..., 0]) and same_bits(got[..., 2].real, power[..., 1])
    assert same_bits(got[..., 1].real, power[..., 2]) and same_bits(got[..., 1].imag, power[..., 3])


def test_in_a_chain_and_through_hdf5(tmp_path, monkeypatch):
    """Three streams stacked in HBM, channelized and correlated; the result written and read back."""
    set_tiling(monkeypatch)
    rng = np.random.default_rng(5)
    n_samp = 16 * 64 * 3 + 40
    xs = [(rng.standard_normal(n_samp) + 1j * rng.standard_normal(n_samp)).astype(np.complex64) for _ in range(3)]

    def channelized():
        return bt.Channelize(bt.Stack([_device(x, samples_per_frame=1024) for x in xs], axis=1), 16)

    spectra = channelized().read()
    assert spectra.shape == (n_samp // 16, 16, 3)
    task = bt.Correlate(channelized(), 64)
    assert task.shape == (3, 16, 6) and task.sample_rate == corr_cases.RATE / 16 / 64
    got = task.read()
    want = bt.correlate_samples(spectra, 64)
    case = corr_cases.Case('chain', (16, 3), -1, 64, 3, spectra.shape[0] - 192)
    ratio = corr_cases.within_bound(got, want, spectra, case)
    print(f'corr error/bound chain: {ratio:.4f}')
    assert ratio <= 1.
    name = str(tmp_path / 'vis.hdf5')
    task.seek(0)
    with hdf5.open(name, 'w', template=task) as fw:
        task.read(out=fw)
        assert fw.tell() == task.shape[0]
    fr = hdf5.open(name)
    assert fr.shape == task.shape and fr.dtype == task.dtype
    assert abs(fr.sample_rate - task.sample_rate) < 1e-9 * task.sample_rate
    assert same_bits(fr.read(), got)
    fr.close()
    task.close()
