"""baseband_tasks_amd: MI355X-native coherent dedispersion and channelization
behind the stream-reader interface of mhvk/baseband-tasks.

The dedispersion -> channelizer hot path and its immediate neighbours
(detection, integration) are provided;
every task here runs hand-written gfx950 kernels through libbbt_hip.so and
raises if that library is missing -- there is no CPU fallback.
"""
from . import units
from .units import Time
from .base import (Base, BaseTaskBase, TaskBase, PaddedTaskBase, Task, SetAttribute, SinglePrecision)
from .generators import (StreamGenerator, EmptyStreamGenerator, Noise, NoiseGenerator,
                         DeviceStream, HostStream, DeviceNoiseGenerator)
from .dm import DispersionMeasure
from .fourier import fft_maker, HipFFTMaker
from .dispersion import Disperse, Dedisperse, DisperseSamples, DedisperseSamples
from .convolution import Convolve, ConvolveSamples
from .sampling import ShiftAndResample, Resample, TimeDelay, ShiftSamples
from .channelize import Channelize, Dechannelize
from .pfb import (sinc_hamming, PolyphaseFilterBank, PolyphaseFilterBankSamples,
                  InversePolyphaseFilterBank)
from .functions import Square, Power
from .integration import Integrate, Fold, PulseStack
from .modulation import Modulate, modulate_samples
from .rfi import SpectralKurtosis, Excise, sk_limits, spectral_kurtosis, excise_flags, excise_samples
from .search import (DMTrials, dm_trial_shifts, dm_trials_samples, Standardize, standardize_samples,
                     BoxcarSearch, boxcar_search_samples, boxcar_candidates, RobustStandardize,
                     robust_standardize_samples, block_median_mad_samples, RunningMedian, Detrend,
                     running_median_samples, detrend_samples)
from . import search
from .periodicity import (fluctuation_spectra, Whiten, whiten_samples, HarmonicSearch, harmonic_search_samples,
                          harmonic_scales, harmonic_candidates, LongSpectra, long_spectra_samples, Accelerate,
                          accelerate_samples, MedianWhiten, median_whiten_samples, median_ratio)
from . import periodicity
from .ffa import (FFASearch, ffa_search_samples, ffa_transform_samples, ffa_shift, ffa_scales, ffa_period,
                  ffa_candidates, ffa_plan)
from . import ffa
from .correlation import Correlate, correlate_samples, baseline_pairs
from . import correlation
from .conversion import Real2Complex
from .shaping import (ChangeSampleShapeBase, ChangeSampleShape, Reshape, Transpose, ReshapeAndTranspose,
                      GetItem, GetSlice)
from .combining import CombineStreamsBase, CombineStreams, Concatenate, Stack
from .ingest import RawFrameStream, open_vdif, open_dada
from . import phases
from . import hip
from . import hdf5
from . import psrfits

__version__ = '0.1.0'
