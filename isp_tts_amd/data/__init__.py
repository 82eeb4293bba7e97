from .features import (AcousticFeatures, collate_audio, melscale_fbanks, pack_filterbank, pitch_frames,  # noqa: F401
                       twiddles, yin_lags)
from .condition import AudioConditioner, Limiter, k_weighting, meter_table, to_pcm16, true_peak_taps  # noqa: F401
from .declip import Declipper  # noqa: F401
from .equalize import (Band, Equalizer, bandpass, deemphasis, equalizer_table, highpass, highshelf, lowpass, lowshelf,  # noqa: F401
                       notch, peaking, preemphasis)
from .noise import NoiseReducer  # noqa: F401
from .pitch import PitchTracker  # noqa: F401
from .resample import AudioFrontEnd, Resampler, compact_taps, resampled_length, sinc_hann_taps  # noqa: F401
from .screen import Screen  # noqa: F401
from .segment import Segmenter  # noqa: F401
from .stretch import PitchShift, TimeStretch, nearest_ratio  # noqa: F401
from .stats import DatasetStats, DatasetStatsResult, FeatureStats  # noqa: F401
